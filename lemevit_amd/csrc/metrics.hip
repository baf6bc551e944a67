// metrics.hip -- the metrics tail of the reference's evaluation loop (engine.py:177-247 validate, validate.py:330-377: nn.CrossEntropyLoss, utils.accuracy(output, target,
// topk=(1, 5)), the --tta reduction output.unfold(0, r, r).mean(dim=2), three reduce_tensor, a synchronize and three .item() per batch):
//   lmv_eval_logits: ONE pass over the logits -> per output row the plain cross-entropy, the rank of the label's class in a stated total order and, optionally, the first
//                    K classes of that order (the predictions);
//   lmv_meter_add  : ONE wave that adds a batch of those per-row results (or a given scalar loss times n) into a persistent float64 DEVICE accumulator.
// Neither synchronises the host, both can be captured.  Bandwidth-trivial; no atomics, every output element has exactly one writer: two runs agree bit for bit.
#include <math.h>
#include "common.h"

// The value of a class (the mean of r logits rows) is recomputed in every sweep: no multiply may be fused into the operation that consumes it, or two sweeps would
// disagree about a value (hipcc contracts a * b - c into one fma by default; it honours this pragma).
#pragma clang fp contract(off)

namespace {
constexpr int EV_WAVES = 4;          // output rows per workgroup: one wave per row

struct EvalArgs {
  const void* logits; const int64_t* labels;
  float* row_loss; int32_t* rank; int32_t* pred;
  int64_t ls;
  int G, N, r, K;          // G = B / r output rows
  float inv_r;
};

// class j of an output row whose first logits row starts at x: (((x_0 + x_1) + ...) + x_{r-1}) * (1 / r) in fp32; r == 1: the logit as it is
template <typename T> __device__ __forceinline__ float ev_value(const T* x, int64_t ls, int r, float inv_r, int j) {
  float v = DT<T>::ld(x + j);
  if (r == 1) return v;
  for (int i = 1; i < r; ++i) v = v + DT<T>::ld(x + i * ls + j);
  return v * inv_r;
}

// A 32-bit key that sorts as the values do: negative values flipped, positive ones above them, -0 = +0, every NaN the top key (torch.topk puts NaN first)
__device__ __forceinline__ uint32_t ev_key(float v) {
  if (v != v) return 0xffffffffu;
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (key, ~index): the LARGER word comes FIRST in the order (greater value, then smaller index).  Never 0: the smallest key, -inf's, is 0x007fffff.
__device__ __forceinline__ unsigned long long ev_word(float v, int j) { return ((unsigned long long)ev_key(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)j); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per output row; 2 + K sweeps over a row (r rows of logits) that stays in cache: max and rank, sum of exponentials, then one sweep per prediction.
template <typename T> __global__ __launch_bounds__(EV_WAVES * LMV_WAVE) void eval_logits_kernel(const EvalArgs a) {
  const int lane = threadIdx.x & (LMV_WAVE - 1);
  const int g = blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
  if (g >= a.G) return;
  const int N = a.N, r = a.r;
  const float inv_r = a.inv_r;
  const int64_t ls = a.ls;
  const T* x = reinterpret_cast<const T*>(a.logits) + (int64_t)g * r * ls;
  const int64_t y64 = a.labels[g];
  if (y64 >= 0 && y64 < N) {
    const int y = (int)y64;
    const float vy = ev_value<T>(x, ls, r, inv_r, y);
    const uint32_t ky = ev_key(vy);
    float mx = -INFINITY;
    int before = 0;
    for (int j = lane; j < N; j += LMV_WAVE) {
      const float v = ev_value<T>(x, ls, r, inv_r, j);
      mx = fmaxf(mx, v);          // (drops a NaN; the sum below keeps it)
      const uint32_t k = ev_key(v);
      before += (k > ky || (k == ky && j < y)) ? 1 : 0;          // at j == y the keys are equal and the index decides: not counted
    }
    mx = wave_max(mx);
    before = wave_sum_i32(before);
    float se = 0.f;
    for (int j = lane; j < N; j += LMV_WAVE) se += expf(ev_value<T>(x, ls, r, inv_r, j) - mx);
    se = wave_sum(se);
    if (lane == 0) { a.row_loss[g] = (mx + logf(se)) - vy; a.rank[g] = before; }
  } else if (lane == 0) {          // ignored row
    a.row_loss[g] = 0.f; a.rank[g] = -1;
  }
  unsigned long long prev = 0ull;
  for (int k = 0; k < a.K; ++k) {          // the best word strictly behind the previous pick; K <= N: there always is one
    unsigned long long best = 0ull;
    for (int j = lane; j < N; j += LMV_WAVE) {
      const unsigned long long w = ev_word(ev_value<T>(x, ls, r, inv_r, j), j);
      if ((k == 0 || w < prev) && w > best) best = w;
    }
    best = wave_max_u64(best);
    prev = best;
    if (lane == 0) a.pred[(int64_t)g * a.K + k] = (int32_t)(0xffffffffu - (uint32_t)best);
  }
}

struct MeterArgs {
  double* state; const float* row_loss; const int32_t* rank; const float* loss;
  double n;
  int rows, nk;
  int32_t k[LMV_METER_MAX_K];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ONE wave: lane l takes rows l, l + 64, ... in order, then the butterfly, all in double (counts are exact there) -- the fixed tree of soft_ce_mean_kernel; then
// one thread adds into the state.  Stream order serialises successive updates.  a.loss != NULL: the scalar mode, state[0] += *loss * n, state[1] += n.
__global__ __launch_bounds__(LMV_WAVE) void meter_add_kernel(const MeterArgs a) {
  if (a.loss) {
    if (threadIdx.x == 0) { a.state[0] += (double)*a.loss * a.n; a.state[1] += a.n; }
    return;
  }
  double ls = 0.0, cnt = 0.0, hits[LMV_METER_MAX_K];
#pragma unroll
  for (int i = 0; i < LMV_METER_MAX_K; ++i) hits[i] = 0.0;
  for (int j = threadIdx.x; j < a.rows; j += LMV_WAVE) {
    const int rk = a.rank[j];
    if (rk < 0) continue;          // ignored row
    ls += (double)a.row_loss[j];
    cnt += 1.0;
#pragma unroll
    for (int i = 0; i < LMV_METER_MAX_K; ++i) hits[i] += (i < a.nk && rk < a.k[i]) ? 1.0 : 0.0;
  }
  ls = wave_sum_f64(ls);
  cnt = wave_sum_f64(cnt);
#pragma unroll
  for (int i = 0; i < LMV_METER_MAX_K; ++i) hits[i] = wave_sum_f64(hits[i]);
  if (threadIdx.x == 0) {
    a.state[0] += ls; a.state[1] += cnt;
#pragma unroll
    for (int i = 0; i < LMV_METER_MAX_K; ++i)
      if (i < a.nk) a.state[2 + i] += hits[i];
  }
}
}  // namespace

extern "C" int lmv_eval_logits(const void* logits, int dtype, int64_t row_stride, int B, int N, const int64_t* labels, int reduce_factor, float* row_loss, int32_t* rank,
                               int32_t* pred, int K, void* stream) {
  if (!logits || !labels || !row_loss || !rank) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: null logits / labels / row_loss / rank");
  if (B < 1 || N < 1) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: bad shape [%d, %d] (B >= 1, N >= 1)", B, N);
  if (reduce_factor < 1 || B % reduce_factor) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: reduce_factor %d must be >= 1 and divide B = %d", reduce_factor, B);
  if (row_stride < N) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: row stride %lld < N = %d", (long long)row_stride, N);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: unsupported logits dtype code %d (fp32 / bf16)", dtype);
  if (K < 0 || K > LMV_EVAL_MAX_PRED) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: K = %d predictions outside 0 .. %d", K, LMV_EVAL_MAX_PRED);
  if (K > N) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: K = %d predictions of N = %d classes", K, N);
  if (K > 0 && !pred) LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: null pred with K = %d", K);
  if ((((uintptr_t)logits) & (dtype == LMV_F32 ? 3u : 1u)) || (((uintptr_t)labels) & 7u) || (((uintptr_t)row_loss) & 3u) || (((uintptr_t)rank) & 3u) || (((uintptr_t)pred) & 3u))
    LMV_FAIL(LMV_ERR_SHAPE, "eval_logits: misaligned buffer");
  EvalArgs a;
  a.logits = logits; a.labels = labels; a.row_loss = row_loss; a.rank = rank; a.pred = pred;
  a.ls = row_stride; a.G = B / reduce_factor; a.N = N; a.r = reduce_factor; a.K = K; a.inv_r = 1.0f / (float)reduce_factor;
  const dim3 grid((a.G + EV_WAVES - 1) / EV_WAVES), block(EV_WAVES * LMV_WAVE);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LMV_F32) hipLaunchKernelGGL(eval_logits_kernel<float>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(eval_logits_kernel<bf16_t>, grid, block, 0, st, a);
  LMV_CHECK_LAUNCH("eval_logits");
  return LMV_OK;
}

extern "C" int lmv_meter_add(double* state, const float* row_loss, const int32_t* rank, int rows, const int32_t* ks, int nk, const float* loss, int64_t n, void* stream) {
  if (!state) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: null state");
  if (nk < 0 || nk > LMV_METER_MAX_K) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: nk = %d thresholds outside 0 .. %d", nk, LMV_METER_MAX_K);
  if (nk > 0 && !ks) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: null ks with nk = %d", nk);
  for (int i = 0; i < nk; ++i)
    if (ks[i] < 1) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: threshold ks[%d] = %d < 1", i, ks[i]);
  const bool per_row = row_loss != nullptr || rank != nullptr;
  if (per_row == (loss != nullptr)) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: exactly one of (row_loss, rank) and loss must be given");
  if (per_row && (!row_loss || !rank)) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: row_loss and rank come together");
  if (per_row && rows < 1) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: rows = %d < 1", rows);
  if (loss && n < 1) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: n = %lld < 1 in the scalar mode", (long long)n);
  if ((((uintptr_t)state) & 7u) || (((uintptr_t)row_loss) & 3u) || (((uintptr_t)rank) & 3u) || (((uintptr_t)loss) & 3u)) LMV_FAIL(LMV_ERR_SHAPE, "meter_add: misaligned buffer");
  MeterArgs a;
  a.state = state; a.row_loss = row_loss; a.rank = rank; a.loss = loss; a.n = (double)n; a.rows = rows; a.nk = nk;
  for (int i = 0; i < LMV_METER_MAX_K; ++i) a.k[i] = i < nk ? ks[i] : 0;
  hipLaunchKernelGGL(meter_add_kernel, dim3(1), dim3(LMV_WAVE), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH("meter_add");
  return LMV_OK;
}
