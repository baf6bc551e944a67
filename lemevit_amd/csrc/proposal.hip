// proposal.hip -- the proposal stage of the oriented RPN head of the Oriented R-CNN configs (upstream OrientedRPNHead.get_bboxes / _get_bboxes_single; its source is
// not part of the reference tree, the rules restate upstream): lmv_rpn_select (+ _workspace_bytes) turns the head's score and regression maps of B images and L
// levels into the per-level top-nms_pre candidates -- row index, level id, sigmoid score, decoded box -- and the global rank order that lmv_obb_nms takes;
// lmv_rpn_gather turns what lmv_obb_nms kept into fixed-shape proposals.  include/lemevit_hip.h has the rules and the semantics.
//
//   choice    level l's K_l slots are the K_l smallest 64-bit words (u << 32) | r over its rows r, u = ~key the complement of the order-preserving image of the
//             fp32 logit (NaN: no candidate): an exact radix select (four 8-bit digits of u, then the row order) and a sort of at most 2 048 words in LDS -- no
//             sort of the level, and no value depends on the order in which an atomic lands (integer counters only): two calls agree bit for bit.
//   launch 1  grid-wide, 2 048 rows per workgroup: u of every row into the workspace (a level's row is padded to 16 entries, so that launch 2 reads them 16 at a
//             time), the histogram of u's top byte per (image, level) in LDS, flushed with integer atomics into a table a memset node zeroed.
//   launch 2  one workgroup of 1 024 threads per (image, level): for an oversubscribed level three more digit sweeps over the workspace give the threshold t and how
//             many rows equal to t to take; one ordered sweep (16 consecutive rows per thread, one block prefix scan of the packed counts) collects the words, a
//             bitonic network sorts them, and every slot gets its index, level id, score and box (the coder's device rule, coder_rules.h: the bits of
//             lmv_box_decode_map).
//   launch 3  one thread per slot: its rank among the image's slots = its slot number in its level + by binary search the slots of every other level in front.
//   gather    one thread per output row of lmv_rpn_gather.
#include "coder_rules.h"          // (switches fp contraction off for the rest of this file, as in coder.hip)
#include "select_frame.h"

namespace {

constexpr int PR_CHUNK = 2048;          // rows per workgroup of launch 1
constexpr int PR_T1 = 256;
constexpr int PR_T2 = 1024, PR_WAVES = PR_T2 / LMV_WAVE;
constexpr int PR_VEC = 16;              // consecutive rows per thread of launch 2; the workspace rows are padded to it
constexpr int PR_SPAN = PR_T2 * PR_VEC;
constexpr uint32_t PR_NONE = 0xffffffffu;          // u of a NaN logit, of a padding entry and of an empty slot: above every candidate's (u <= 0xff800000, -inf)
constexpr size_t PR_HIST_BYTES = LMV_RPN_LOSS_MAX_LEVELS * 256 * sizeof(uint32_t);          // per image

static_assert(PR_T1 == 256, "launch 1 clears and flushes one histogram bin per thread");
static_assert(PR_SPAN <= 65535, "launch 2 scans two 16-bit counts in one word");
static_assert(LMV_RPN_MAX_PRE == 2 * PR_T2, "the sort network and the slot loop of launch 2");
static_assert(LMV_RPN_LOSS_MAX_LEVELS * LMV_RPN_MAX_PRE <= LMV_OBB_NMS_MAX, "Ktot <= LMV_OBB_NMS_MAX follows from the two limits");

__host__ __device__ inline int pr_padded(int n) { return (n + PR_VEC - 1) / PR_VEC * PR_VEC; }

struct PrMap { const void* p; int64_t sb, sc, sh, sw; };
struct PrLevel {
  PrMap cls, reg;
  int H, W, n, np, K;          // n = H W A rows, np = n padded to 16, K = min(nms_pre, n) slots
  int off, woff, koff;         // the level's first anchor, first workspace entry, first slot
  int c0;                      // its first workgroup of launch 1
};

struct PrArgs {
  PrLevel lv[LMV_RPN_LOSS_MAX_LEVELS];
  int L, A, Np, Ktot;
  const float* anchors; int anchor_stride;
  CdNorm nm; float max_ratio, min_size;
  uint32_t* hist; uint32_t* ukeys; uint32_t* skeys;          // the workspace: [B, 5, 256], [B, Np], [B, Ktot]
  int64_t* index; int32_t* groups; float* scores; float* boxes; int64_t* order;
};

// logit -> u: the smaller, the better.  key = the order-preserving image of the fp32 value (-0.0 counts as +0.0), u = ~key; NaN -> PR_NONE
__device__ __forceinline__ uint32_t pr_u(float z) {
  if (z != z) return PR_NONE;
  const uint32_t bits = z == 0.f ? 0u : __float_as_uint(z);
  return (bits & 0x80000000u) ? bits : (~bits & 0x7fffffffu);
}
__device__ __forceinline__ float pr_logit(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? u : (~u & 0x7fffffffu)); }

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PR_T1) void rpn_key_kernel(PrArgs a) {
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x, b = blockIdx.y;
  h[tid] = 0u;
  __syncthreads();
  int l = 0;
#pragma unroll
  for (int i = 1; i < LMV_RPN_LOSS_MAX_LEVELS; ++i) l += (i < a.L && (int)blockIdx.x >= a.lv[i].c0) ? 1 : 0;
  const PrLevel& lv = a.lv[l];
  const T* cls = (const T*)lv.cls.p + b * lv.cls.sb;
  uint32_t* out = a.ukeys + (int64_t)b * a.Np + lv.woff;
  const int base = ((int)blockIdx.x - lv.c0) * PR_CHUNK;
#pragma unroll
  for (int i = 0; i < PR_CHUNK / PR_T1; ++i) {
    const int e = base + i * PR_T1 + tid;
    if (e < lv.np) {
      uint32_t u = PR_NONE;
      if (e < lv.n) {
        const int pos = e / a.A, an = e - pos * a.A, y = pos / lv.W, x = pos - y * lv.W;
        u = pr_u(DT<T>::ld(cls + an * lv.cls.sc + y * lv.cls.sh + x * lv.cls.sw));
        if (u != PR_NONE) atomicAdd(&h[u >> 24], 1u);
      }
      out[e] = u;
    }
  }
  __syncthreads();
  const uint32_t v = h[tid];
  if (v) atomicAdd(&a.hist[((int64_t)b * LMV_RPN_LOSS_MAX_LEVELS + l) * 256 + tid], v);
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
// entries e0 .. e0 + 15 of a padded workspace row (e0 % 16 == 0): four 16-byte loads
__device__ __forceinline__ void pr_load(const uint32_t* __restrict__ keys, int e0, uint32_t* u) {
#pragma unroll
  for (int q = 0; q < PR_VEC / 4; ++q) {
    const uint4 v = reinterpret_cast<const uint4*>(keys + e0)[q];
    u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
  }
}

template <typename T>
__global__ __launch_bounds__(PR_T2) void rpn_select_kernel(PrArgs a) {
  __shared__ uint32_t h[256];
  __shared__ uint32_t wt[2][PR_WAVES];          // [parity of the iteration][wave]
  __shared__ uint32_t s_cnt, s_pref, s_rest;
  __shared__ unsigned long long words[LMV_RPN_MAX_PRE];
  const int tid = threadIdx.x, lane = tid & (LMV_WAVE - 1), wave = tid >> 6, l = blockIdx.x, b = blockIdx.y;
  const PrLevel& lv = a.lv[l];
  const uint32_t* keys = a.ukeys + (int64_t)b * a.Np + lv.woff;
  if (tid < 256) h[tid] = a.hist[((int64_t)b * LMV_RPN_LOSS_MAX_LEVELS + l) * 256 + tid];
  if (tid == 0) { s_pref = PR_NONE; s_rest = 0u; }          // what holds when every candidate is taken: all of them are below the threshold
  __syncthreads();
  if (wave == 0) {          // the bin total is the number of candidates
    uint32_t s = (h[4 * lane] + h[4 * lane + 1]) + (h[4 * lane + 2] + h[4 * lane + 3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, LMV_WAVE);
    if (lane == 0) s_cnt = s;
  }
  __syncthreads();
  const int cand = (int)min(s_cnt, (uint32_t)lv.n), take = min(lv.K, cand);
  const bool some = cand > lv.K;          // (workgroup-uniform)
  if (some) {          // the threshold, digit by digit; s_rest: how many to take among the rows that share the digits so far
    if (wave == 0) {
      uint32_t bin = 0u, rest = 0u;
      lmv_select_pick(h, (uint32_t)take, lane, &bin, &rest);
      if (rest) { s_pref = bin << 24; s_rest = rest; }          // (the finding lane alone: rest >= 1 there, 0 elsewhere)
    }
    for (int shift = 16; shift >= 0; shift -= 8) {
      __syncthreads();
      if (tid < 256) h[tid] = 0u;
      __syncthreads();
      const uint32_t pf = s_pref >> (shift + 8);
      for (int e0 = tid * PR_VEC; e0 < lv.np; e0 += PR_SPAN) {
        uint32_t u[PR_VEC];
        pr_load(keys, e0, u);
#pragma unroll
        for (int j = 0; j < PR_VEC; ++j)
          if (u[j] != PR_NONE && (u[j] >> (shift + 8)) == pf) atomicAdd(&h[(u[j] >> shift) & 0xffu], 1u);
      }
      __syncthreads();
      if (wave == 0) {
        uint32_t bin = 0u, rest = 0u;
        const uint32_t r = s_rest;
        lmv_select_pick(h, r, lane, &bin, &rest);
        if (rest) { s_pref = (s_pref & ~(0xffu << shift)) | (bin << shift); s_rest = rest; }
      }
    }
    __syncthreads();
  }
  const uint32_t t = s_pref;
  const int rest = (int)s_rest, n_less = take - rest;
  // the words of the chosen rows: those below t in row order, then the first `rest` rows equal to t in row order
  int less_before = 0, eq_before = 0, parity = 0;
  for (int base = 0; base < lv.np; base += PR_SPAN, parity ^= 1) {
    const int e0 = base + tid * PR_VEC;
    uint32_t u[PR_VEC];
    if (e0 < lv.np) pr_load(keys, e0, u);
    else {
#pragma unroll
      for (int j = 0; j < PR_VEC; ++j) u[j] = PR_NONE;
    }
    uint32_t mine = 0u, total;
#pragma unroll
    for (int j = 0; j < PR_VEC; ++j) {
      if (u[j] < t) mine += 1u;
      else if (some && u[j] == t) mine += 1u << 16;
    }
    const uint32_t ex = lmv_select_scan<PR_WAVES>(mine, wt[parity], lane, wave, &total);
    int at = less_before + (int)(ex & 0xffffu), eq = eq_before + (int)(ex >> 16);
    less_before += (int)(total & 0xffffu); eq_before += (int)(total >> 16);
#pragma unroll
    for (int j = 0; j < PR_VEC; ++j) {
      const unsigned long long w = ((unsigned long long)u[j] << 32) | (unsigned)(e0 + j);
      if (u[j] < t) {
        if (at < n_less) words[at] = w;          // (always: the counts come from the same keys)
        ++at;
      } else if (some && u[j] == t) {
        if (eq < rest) words[n_less + eq] = w;
        ++eq;
      }
    }
  }
  int P = 2;
  while (P < take) P <<= 1;          // (take <= LMV_RPN_MAX_PRE, a power of two)
  for (int i = take + tid; i < P; i += PR_T2) words[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += PR_T2) {
        const int m = i ^ j;
        if (m > i) {
          const unsigned long long x = words[i], y = words[m];
          if ((x > y) == ((i & k) == 0)) { words[i] = y; words[m] = x; }
        }
      }
      __syncthreads();
    }
  }
  // the slots
  const T* reg = (const T*)lv.reg.p + b * lv.reg.sb;
  for (int s = tid; s < lv.K; s += PR_T2) {
    const int64_t g = (int64_t)b * a.Ktot + lv.koff + s;
    int64_t r = -1;
    uint32_t u = PR_NONE;
    float score = -INFINITY, o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (s < take) {
      const unsigned long long w = words[s];
      u = (uint32_t)(w >> 32);
      const int row = (int)(uint32_t)w;
      r = row;
      const float z = pr_logit(u);
      score = 1.f / (1.f + expf(-z));
      const int pos = row / a.A, an = row - pos * a.A, y = pos / lv.W, x = pos - y * lv.W;
      const float* pb = a.anchors + (int64_t)(lv.off + row) * a.anchor_stride;
      const T* db = reg + (int64_t)an * 6 * lv.reg.sc + y * lv.reg.sh + x * lv.reg.sw;
      float p[4], d[6];
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = pb[j];
#pragma unroll
      for (int j = 0; j < 6; ++j) d[j] = DT<T>::ld(db + j * lv.reg.sc);
      cd_midpoint_decode(p, d, a.nm, a.max_ratio, o);
      if (a.min_size > 0.f && !(o[2] >= a.min_size && o[3] >= a.min_size)) score = -INFINITY;          // upstream keeps (w >= min) & (h >= min)
    }
    a.index[g] = r;
    a.groups[g] = l;
    a.scores[g] = score;
    a.skeys[g] = u;
    float* bo = a.boxes + g * 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) bo[j] = o[j];
  }
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
// the entries of the ascending k[0 .. n) that are < u (or_equal == false) or <= u (true)
__device__ __forceinline__ int pr_count(const uint32_t* __restrict__ k, int n, uint32_t u, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t v = k[mid];
    if (or_equal ? v <= u : v < u) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void rpn_order_kernel(PrArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (s >= a.Ktot) return;
  const uint32_t* k = a.skeys + (int64_t)b * a.Ktot;
  int l = 0;
#pragma unroll
  for (int i = 1; i < LMV_RPN_LOSS_MAX_LEVELS; ++i) l += (i < a.L && s >= a.lv[i].koff) ? 1 : 0;
  const uint32_t u = k[s];
  int rank = 0;
#pragma unroll
  for (int i = 0; i < LMV_RPN_LOSS_MAX_LEVELS; ++i) {
    if (i >= a.L) continue;
    const int ko = a.lv[i].koff, K = a.lv[i].K;
    rank += i == l ? s - ko : pr_count(k + ko, K, u, i < l);          // on equal keys the lower level is in front; empty slots (PR_NONE) come last
  }
  a.order[(int64_t)b * a.Ktot + rank] = s;
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rpn_gather_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, int Ktot, const int64_t* __restrict__ keep,
                                                         const int64_t* __restrict__ count, int max_num, float* __restrict__ proposals, float* __restrict__ out_scores,
                                                         int32_t* __restrict__ num, uint8_t* __restrict__ ignore) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int64_t c = min(max(count[b], (int64_t)0), (int64_t)max_num);
  if (i == 0) num[b] = (int32_t)c;
  if (i >= max_num) return;
  const int64_t o = (int64_t)b * max_num + i;
  const int64_t k = i < c ? keep[o] : -1;
  const bool live = k >= 0 && k < (int64_t)Ktot;          // (a kept entry always is; anything else reads nothing and is padding)
  float row[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, sc = -INFINITY;
  if (live) {
    const float* src = boxes + ((int64_t)b * Ktot + k) * 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) row[j] = src[j];
    sc = scores[(int64_t)b * Ktot + k];
  }
  float* dst = proposals + o * 5;
#pragma unroll
  for (int j = 0; j < 5; ++j) dst[j] = row[j];
  out_scores[o] = sc;
  ignore[o] = live ? 0 : 1;
}

// ---- host checks ------------------------------------------------------------------------------------------------------------------------------------------------
bool pr_misaligned(const void* p, unsigned bytes) { return (((uintptr_t)p) & (bytes - 1u)) != 0; }

// the sizes that the workspace and the outputs follow from; `fn` names the caller in the message
int pr_sizes(const char* fn, const int32_t* H, const int32_t* W, int L, int A, int B, int nms_pre, int64_t* N, int64_t* Np, int* Ktot) {
  if (L < 1 || L > LMV_RPN_LOSS_MAX_LEVELS) LMV_FAIL(LMV_ERR_SHAPE, "%s: L = %d levels outside 1 .. %d", fn, L, LMV_RPN_LOSS_MAX_LEVELS);
  if (A < 1 || A > LMV_CODER_MAX_SETS) LMV_FAIL(LMV_ERR_SHAPE, "%s: A = %d anchors per position outside 1 .. %d", fn, A, LMV_CODER_MAX_SETS);
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (nms_pre < 1 || nms_pre > LMV_RPN_MAX_PRE) LMV_FAIL(LMV_ERR_SHAPE, "%s: nms_pre = %d outside 1 .. %d", fn, nms_pre, LMV_RPN_MAX_PRE);
  *N = 0; *Np = 0; *Ktot = 0;
  for (int l = 0; l < L; ++l) {
    if (H[l] < 1 || W[l] < 1 || (int64_t)H[l] * W[l] > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: a map of %d x %d positions (each at least 1)", fn, l, H[l], W[l]);
    const int64_t n = (int64_t)H[l] * W[l] * A;
    *N += n;
    if (*N > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = sum H W A exceeds %d anchors per image", fn, LMV_OBB_MAX_BOXES);
    *Np += pr_padded((int)n);
    *Ktot += (int)(n < nms_pre ? n : nms_pre);
  }
  if (*Ktot > LMV_OBB_NMS_MAX) LMV_FAIL(LMV_ERR_SHAPE, "%s: Ktot = %d slots per image, at most %d", fn, *Ktot, LMV_OBB_NMS_MAX);
  return LMV_OK;
}

size_t pr_bytes(int B, int64_t Np, int Ktot) { return (size_t)B * (PR_HIST_BYTES + (size_t)Np * 4 + (size_t)Ktot * 4); }

// a map [B, Ch, H, W] through its strides: non-null, aligned to its element, positive strides, the images apart by at least one image's extent (headloss.hip's rule)
int pr_map(const char* fn, const char* what, int l, const void* p, const int64_t* s, int B, int Ch, int H, int W, unsigned esize) {
  if (!p) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: null %s map", fn, l, what);
  if (pr_misaligned(p, esize)) LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: misaligned %s map", fn, l, what);
  const int64_t extent = 1 + (int64_t)(Ch - 1) * s[1] + (int64_t)(H - 1) * s[2] + (int64_t)(W - 1) * s[3];
  if (s[1] < 1 || s[2] < 1 || s[3] < 1 || (B > 1 && s[0] < extent))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: level %d: %s map: strides (%lld, %lld, %lld, %lld) smaller than the extent of [%d, %d, %d, %d]", fn, l, what, (long long)s[0],
             (long long)s[1], (long long)s[2], (long long)s[3], B, Ch, H, W);
  return LMV_OK;
}

}  // namespace

extern "C" size_t lmv_rpn_select_workspace_bytes(const int32_t* sizes, int L, int A, int B, int nms_pre) {
  if (!sizes || L < 1 || L > LMV_RPN_LOSS_MAX_LEVELS) return 0;
  int32_t H[LMV_RPN_LOSS_MAX_LEVELS], W[LMV_RPN_LOSS_MAX_LEVELS];
  for (int l = 0; l < L; ++l) { H[l] = sizes[2 * l]; W[l] = sizes[2 * l + 1]; }
  int64_t N, Np;
  int Ktot;
  if (pr_sizes("rpn_select_workspace_bytes", H, W, L, A, B, nms_pre, &N, &Np, &Ktot)) return 0;
  return pr_bytes(B, Np, Ktot);
}

extern "C" int lmv_rpn_select(const lmv_rpn_loss_level* levels, int L, int A, int dtype, int B, const float* anchors, int anchor_stride, int nms_pre,
                              float min_bbox_size, const float* means, const float* stds, float wh_ratio_clip, void* workspace, size_t workspace_bytes, int64_t* index,
                              int32_t* groups, float* scores, float* boxes, int64_t* order, void* stream) {
  const char* fn = "rpn_select";
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown dtype %d (LMV_F32 / LMV_BF16)", fn, dtype);
  if (L < 1 || L > LMV_RPN_LOSS_MAX_LEVELS || !levels) LMV_FAIL(LMV_ERR_SHAPE, "%s: L = %d levels outside 1 .. %d, or a null level table", fn, L, LMV_RPN_LOSS_MAX_LEVELS);
  int32_t H[LMV_RPN_LOSS_MAX_LEVELS], W[LMV_RPN_LOSS_MAX_LEVELS];
  for (int l = 0; l < L; ++l) { H[l] = levels[l].H; W[l] = levels[l].W; }
  int64_t N, Np;
  int Ktot;
  if (int rc = pr_sizes(fn, H, W, L, A, B, nms_pre, &N, &Np, &Ktot)) return rc;
  if (anchor_stride < 4) LMV_FAIL(LMV_ERR_SHAPE, "%s: an anchor row stride of %d floats, at least 4", fn, anchor_stride);
  if (min_bbox_size != min_bbox_size || min_bbox_size < 0.f) LMV_FAIL(LMV_ERR_SHAPE, "%s: min_bbox_size = %g is negative or NaN (0: no rule)", fn, min_bbox_size);
  if (!(wh_ratio_clip > 0.f) || !isfinite(wh_ratio_clip)) LMV_FAIL(LMV_ERR_SHAPE, "%s: wh_ratio_clip = %g is not a positive finite number", fn, wh_ratio_clip);
  if (!means || !stds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null means / stds (host arrays of 6 floats)", fn);
  PrArgs a;
  for (int i = 0; i < CD_MAX_D; ++i) {
    a.nm.mean[i] = means[i]; a.nm.std[i] = stds[i];
    if (means[i] != means[i] || stds[i] != stds[i]) LMV_FAIL(LMV_ERR_SHAPE, "%s: a NaN mean or std (entry %d)", fn, i);
  }
  const unsigned esize = dtype == LMV_F32 ? 4u : 2u;
  int off = 0, woff = 0, koff = 0, c0 = 0;
  for (int l = 0; l < L; ++l) {
    const lmv_rpn_loss_level& s = levels[l];
    if (int rc = pr_map(fn, "class", l, s.cls, s.cls_stride, B, A, s.H, s.W, esize)) return rc;
    if (int rc = pr_map(fn, "regression", l, s.reg, s.reg_stride, B, A * 6, s.H, s.W, esize)) return rc;
    PrLevel& v = a.lv[l];
    v.cls = PrMap{s.cls, s.cls_stride[0], s.cls_stride[1], s.cls_stride[2], s.cls_stride[3]};
    v.reg = PrMap{s.reg, s.reg_stride[0], s.reg_stride[1], s.reg_stride[2], s.reg_stride[3]};
    v.H = s.H; v.W = s.W; v.n = s.H * s.W * A; v.np = pr_padded(v.n); v.K = v.n < nms_pre ? v.n : nms_pre;
    v.off = off; v.woff = woff; v.koff = koff; v.c0 = c0;
    off += v.n; woff += v.np; koff += v.K; c0 += (v.np + PR_CHUNK - 1) / PR_CHUNK;
  }
  for (int l = L; l < LMV_RPN_LOSS_MAX_LEVELS; ++l) { a.lv[l] = a.lv[0]; a.lv[l].n = a.lv[l].np = a.lv[l].K = 0; a.lv[l].off = off; a.lv[l].woff = woff; a.lv[l].koff = koff; a.lv[l].c0 = c0; }
  if (!anchors || !index || !groups || !scores || !boxes || !order) LMV_FAIL(LMV_ERR_SHAPE, "%s: null anchors / index / groups / scores / boxes / order", fn);
  if (pr_misaligned(anchors, 4) || pr_misaligned(groups, 4) || pr_misaligned(scores, 4) || pr_misaligned(boxes, 4) || pr_misaligned(index, 8) || pr_misaligned(order, 8) ||
      pr_misaligned(workspace, 16))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer (the workspace: 16 bytes)", fn);
  const size_t need = pr_bytes(B, Np, Ktot);
  if (workspace_bytes < need || !workspace) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (lmv_rpn_select_workspace_bytes)", fn, workspace_bytes, need);
  a.L = L; a.A = A; a.Np = (int)Np; a.Ktot = Ktot;
  a.anchors = anchors; a.anchor_stride = anchor_stride;
  a.max_ratio = (float)fabs(log((double)wh_ratio_clip)); a.min_size = min_bbox_size;
  a.hist = reinterpret_cast<uint32_t*>(workspace);
  a.ukeys = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + (size_t)B * PR_HIST_BYTES);
  a.skeys = a.ukeys + (size_t)B * Np;
  a.index = index; a.groups = groups; a.scores = scores; a.boxes = boxes; a.order = order;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, (size_t)B * PR_HIST_BYTES, st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot clear the histograms", fn);
  const dim3 g1((unsigned)c0, (unsigned)B), g2((unsigned)L, (unsigned)B), g3((unsigned)((Ktot + 255) / 256), (unsigned)B);
  if (dtype == LMV_F32) hipLaunchKernelGGL(rpn_key_kernel<float>, g1, dim3(PR_T1), 0, st, a);
  else hipLaunchKernelGGL(rpn_key_kernel<bf16_t>, g1, dim3(PR_T1), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  if (dtype == LMV_F32) hipLaunchKernelGGL(rpn_select_kernel<float>, g2, dim3(PR_T2), 0, st, a);
  else hipLaunchKernelGGL(rpn_select_kernel<bf16_t>, g2, dim3(PR_T2), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(rpn_order_kernel, g3, dim3(256), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_rpn_gather(const float* boxes, const float* scores, int Ktot, const int64_t* keep, const int64_t* count, int B, int max_num, float* proposals,
                              float* out_scores, int32_t* num, uint8_t* ignore, void* stream) {
  const char* fn = "rpn_gather";
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (Ktot < 1 || Ktot > LMV_OBB_NMS_MAX) LMV_FAIL(LMV_ERR_SHAPE, "%s: Ktot = %d slots per image outside 1 .. %d", fn, Ktot, LMV_OBB_NMS_MAX);
  if (max_num < 1 || max_num > LMV_OBB_NMS_MAX) LMV_FAIL(LMV_ERR_SHAPE, "%s: max_num = %d outside 1 .. %d", fn, max_num, LMV_OBB_NMS_MAX);
  if (!boxes || !scores || !keep || !count || !proposals || !out_scores || !num || !ignore)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes / scores / keep / count / proposals / scores out / num / ignore", fn);
  if (pr_misaligned(boxes, 4) || pr_misaligned(scores, 4) || pr_misaligned(proposals, 4) || pr_misaligned(out_scores, 4) || pr_misaligned(num, 4) || pr_misaligned(keep, 8) ||
      pr_misaligned(count, 8))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  hipLaunchKernelGGL(rpn_gather_kernel, dim3((unsigned)((max_num + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, boxes, scores, Ktot, keep, count, max_num,
                     proposals, out_scores, num, ignore);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
