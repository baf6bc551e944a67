// attnmap.hip -- the attention probabilities of an lmv_attn_fwd call, written out (lmv_attn_probs).
//
// The forward kernels are flash-style: they keep o and the per-row log-sum-exp, the probabilities never exist.  This file recomputes
//   P[b,h,i,j] = exp(scale * q[b,i,h,:] . k[b,j,h,:] - lse[b,h,i])
// from the packed projections IN PLACE (same (batch, row) strides as the forward) -- the recomputation the backward kernels do
// internally, with P stored instead of consumed.  One pass, no workspace, no atomics; every element of p is written exactly once.
//
// The kernel moves 4 B per probability against 2 x 64 B per key row: it is write-bound, and the shape of the stores decides its speed.
// A 16 x 16 MFMA score tile D[key][query] leaves a lane with 4 consecutive keys of ONE query, i.e. 16 lanes in 16 different rows.
//   general (16 queries x 256 keys per workgroup, 64 keys per wave): the wave's 16 x 64 tile goes through LDS and leaves as
//     256-byte row pieces (16 lanes x 16 B along the key index; 4-byte stores along the key index when Lk is not a multiple of 4).
//     <= 16 queries over many keys (meta over image) is this kernel with one query tile: the key ranges are the parallelism, and with
//     the log-sum-exp given there is nothing to combine.
//   few keys (Lk <= 16; image over meta): a P row is Lk * 4 <= 64 B and consecutive rows are contiguous, so the accumulator as it
//     stands is already right: at Lk = 16 a wave instruction stores 16 rows x 64 B = 1 KiB contiguous.
// head_mean: the workgroup that owns an output tile loops h = 0 .. H-1 itself and sums in that order -> bit-identical run to run.
// bf16 scores: one v_mfma_f32_16x16x32_bf16 per 16 x 16 tile (head dim 32 = the whole contraction).  fp32: exact FMAs, as csrc/attn.hip.
#include "common.h"

namespace {

constexpr int D = 32;
constexpr int TQ = 16;     // queries per tile
constexpr int TK = 256;    // keys per workgroup in the general kernels (64 per wave)
constexpr int QW = 256;    // queries per workgroup in the few-key kernels (64 per wave)
constexpr int LDP = 68;    // floats per row of a wave's 16 x 64 transposition tile (272 B: 16-byte aligned rows, conflict-free float4 writes)

struct ProbArgs {
  const void* q; const void* k; const float* lse; float* p;
  int64_t q_bs, q_rs, k_bs, k_rs;
  int B, H, Lq, Lk;
  float scale, inv_h;
};

// MFMA operand fragment: row `row` of a strided [L][32] bf16 matrix, the 8 elements at 8 * g (rows >= L are zero)
__device__ __forceinline__ bf16x8_t load_frag(const bf16_t* base, int64_t rs, int row, int L, int g) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (row < L) v = *reinterpret_cast<const uint4*>(base + (int64_t)row * rs + g * 8);
  return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ void load_row_f32(const float* p, float* f) {
#pragma unroll
  for (int c = 0; c < D / 4; ++c) chunk_to_f<float>(*reinterpret_cast<const uint4*>(p + c * 4), f + c * 4);
}

// rows [r0, r0 + 16) of a strided [L][32] fp32 matrix -> LDS [16][32]; rows >= L are zero  (threads 0 .. 127)
__device__ __forceinline__ void load_tile16_f32(float* s, const float* base, int64_t rs, int r0, int L, int tid) {
  if (tid < TQ * (D / 4)) {
    const int r = tid >> 3, cc = tid & 7;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < L) v = *reinterpret_cast<const float4*>(base + (int64_t)(r0 + r) * rs + cc * 4);
    *reinterpret_cast<float4*>(s + r * D + cc * 4) = v;
  }
}

__device__ __forceinline__ float dot32(const float* a_reg, const float* s_row) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    const float4 kv = *reinterpret_cast<const float4*>(s_row + d);
    acc += a_reg[d] * kv.x + a_reg[d + 1] * kv.y + a_reg[d + 2] * kv.z + a_reg[d + 3] * kv.w;
  }
  return acc;
}

// the (batch, first head, head count) of the output plane blockIdx.z / .y `plane`
template <bool MEAN>
__device__ __forceinline__ void plane_of(const ProbArgs& a, int plane, int& b, int& h0, int& nh) {
  if (MEAN) { b = plane; h0 = 0; nh = a.H; }
  else { b = plane / a.H; h0 = plane - b * a.H; nh = 1; }
}

// =============================================================================================
// bf16, general: grid (key tiles of 256, query tiles of 16, planes)
// =============================================================================================
template <bool MEAN>
__global__ __launch_bounds__(256) void probs_mfma_kernel(const ProbArgs a) {
  __shared__ __attribute__((aligned(16))) float sP[4][TQ * LDP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int q0 = blockIdx.y * TQ, k0 = blockIdx.x * TK + wave * 64;
  int b, h0, nh;
  plane_of<MEAN>(a, blockIdx.z, b, h0, nh);
  const bool live = k0 < a.Lk;                      // wave-uniform
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  f32x4_t acc[4] = {zero, zero, zero, zero};      // acc[t][r]: key k0 + 16 t + 4 g + r of query q0 + c
  if (live) {
    const int qi = q0 + c;
    for (int hh = 0; hh < nh; ++hh) {
      const int h = h0 + hh;
      const bf16_t* qb = reinterpret_cast<const bf16_t*>(a.q) + b * a.q_bs + h * D;
      const bf16_t* kb = reinterpret_cast<const bf16_t*>(a.k) + b * a.k_bs + h * D;
      const bf16x8_t qf = load_frag(qb, a.q_rs, qi, a.Lq, g);
      const float l = qi < a.Lq ? a.lse[((int64_t)b * a.H + h) * a.Lq + qi] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8_t kf = load_frag(kb, a.k_rs, k0 + t * 16 + c, a.Lk, g);
        const f32x4_t s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, zero, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(fmaf(a.scale, s[r], -l));
          acc[t][r] = MEAN ? acc[t][r] + p : p;
        }
      }
    }
  }
  float* sp = sP[wave];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f32x4_t v = MEAN ? acc[t] * a.inv_h : acc[t];
    *reinterpret_cast<float4*>(sp + c * LDP + t * 16 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  if (!live) return;
  float* pb = a.p + (int64_t)blockIdx.z * a.Lq * a.Lk;
  if ((a.Lk & 3) == 0) {            // 16 lanes x 16 B = 256 contiguous bytes of a row, 4 rows per instruction
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int row = pass * 4 + g, col = c * 4;
      if (q0 + row < a.Lq && k0 + col < a.Lk)
        *reinterpret_cast<float4*>(pb + (int64_t)(q0 + row) * a.Lk + k0 + col) = *reinterpret_cast<const float4*>(sp + row * LDP + col);
    }
  } else {                          // rows are not 16-byte aligned: 64 lanes x 4 B along the key index
    const bool kok = k0 + lane < a.Lk;
#pragma unroll
    for (int row = 0; row < TQ; ++row)
      if (kok && q0 + row < a.Lq) pb[(int64_t)(q0 + row) * a.Lk + k0 + lane] = sp[row * LDP + lane];
  }
}

// =============================================================================================
// bf16, Lk <= 16: grid (query ranges of 256, planes); a wave owns 64 queries
// =============================================================================================
template <bool MEAN>
__global__ __launch_bounds__(256) void probs_mfma_fewk_kernel(const ProbArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int q0 = blockIdx.x * QW + wave * 64;
  if (q0 >= a.Lq) return;
  int b, h0, nh;
  plane_of<MEAN>(a, blockIdx.y, b, h0, nh);
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  f32x4_t acc[4] = {zero, zero, zero, zero};      // acc[t][r]: key 4 g + r of query q0 + 16 t + c
  for (int hh = 0; hh < nh; ++hh) {
    const int h = h0 + hh;
    const bf16_t* qb = reinterpret_cast<const bf16_t*>(a.q) + b * a.q_bs + h * D;
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(a.k) + b * a.k_bs + h * D;
    const bf16x8_t kf = load_frag(kb, a.k_rs, c, a.Lk, g);
    const float* lb = a.lse + ((int64_t)b * a.H + h) * a.Lq;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int qi = q0 + t * 16 + c;
      const bf16x8_t qf = load_frag(qb, a.q_rs, qi, a.Lq, g);
      const float l = qi < a.Lq ? lb[qi] : 0.f;
      const f32x4_t s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, zero, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(fmaf(a.scale, s[r], -l));
        acc[t][r] = MEAN ? acc[t][r] + p : p;
      }
    }
  }
  float* pb = a.p + (int64_t)blockIdx.y * a.Lq * a.Lk;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int qi = q0 + t * 16 + c;
    if (qi >= a.Lq) continue;
    const f32x4_t v = MEAN ? acc[t] * a.inv_h : acc[t];
    if (a.Lk == 16) {                // 16 rows x 64 B = 1 KiB contiguous per wave instruction
      *reinterpret_cast<float4*>(pb + (int64_t)qi * 16 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < a.Lk) pb[(int64_t)qi * a.Lk + 4 * g + r] = v[r];
    }
  }
}

// =============================================================================================
// fp32, general: one key per lane, the 16 queries of the tile broadcast from LDS; grid as probs_mfma_kernel
// =============================================================================================
template <bool MEAN>
__global__ __launch_bounds__(256) void probs_f32_kernel(const ProbArgs a) {
  __shared__ __attribute__((aligned(16))) float sQ[TQ * D];
  __shared__ float sL[TQ];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.y * TQ, j = blockIdx.x * TK + tid;
  const bool valid = j < a.Lk;
  int b, h0, nh;
  plane_of<MEAN>(a, blockIdx.z, b, h0, nh);
  float* pb = a.p + (int64_t)blockIdx.z * a.Lq * a.Lk;
  float acc[TQ];
#pragma unroll
  for (int i = 0; i < TQ; ++i) acc[i] = 0.f;
  for (int hh = 0; hh < nh; ++hh) {
    const int h = h0 + hh;
    const float* qb = reinterpret_cast<const float*>(a.q) + b * a.q_bs + h * D;
    const float* kb = reinterpret_cast<const float*>(a.k) + b * a.k_bs + h * D;
    __syncthreads();
    load_tile16_f32(sQ, qb, a.q_rs, q0, a.Lq, tid);
    if (tid < TQ) sL[tid] = q0 + tid < a.Lq ? a.lse[((int64_t)b * a.H + h) * a.Lq + q0 + tid] : 0.f;
    float kr[D];
    if (valid) load_row_f32(kb + (int64_t)j * a.k_rs, kr);
#pragma unroll
    for (int d = 0; d < D; ++d) { if (!valid) kr[d] = 0.f; }
    __syncthreads();
    if (MEAN) {
#pragma unroll
      for (int i = 0; i < TQ; ++i) acc[i] += expf(dot32(kr, sQ + i * D) * a.scale - sL[i]);
    } else {                         // one head: store as computed (64 lanes x 4 B = 256 contiguous bytes of row q0 + i)
#pragma unroll 2
      for (int i = 0; i < TQ; ++i) {
        const float p = expf(dot32(kr, sQ + i * D) * a.scale - sL[i]);
        if (valid && q0 + i < a.Lq) pb[(int64_t)(q0 + i) * a.Lk + j] = p;
      }
    }
  }
  if (!MEAN || !valid) return;
#pragma unroll
  for (int i = 0; i < TQ; ++i)
    if (q0 + i < a.Lq) pb[(int64_t)(q0 + i) * a.Lk + j] = acc[i] * a.inv_h;
}

// =============================================================================================
// fp32, Lk <= 16: one query per lane, the keys broadcast from LDS; grid as probs_mfma_fewk_kernel
// =============================================================================================
template <bool MEAN>
__global__ __launch_bounds__(256) void probs_f32_fewk_kernel(const ProbArgs a) {
  __shared__ __attribute__((aligned(16))) float sK[TQ * D];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * QW + tid;
  const bool valid = i < a.Lq;
  int b, h0, nh;
  plane_of<MEAN>(a, blockIdx.y, b, h0, nh);
  float acc[TQ];
#pragma unroll
  for (int j = 0; j < TQ; ++j) acc[j] = 0.f;
  for (int hh = 0; hh < nh; ++hh) {
    const int h = h0 + hh;
    const float* qb = reinterpret_cast<const float*>(a.q) + b * a.q_bs + h * D;
    const float* kb = reinterpret_cast<const float*>(a.k) + b * a.k_bs + h * D;
    __syncthreads();
    load_tile16_f32(sK, kb, a.k_rs, 0, a.Lk, tid);
    float q[D], l = 0.f;
    if (valid) { load_row_f32(qb + (int64_t)i * a.q_rs, q); l = a.lse[((int64_t)b * a.H + h) * a.Lq + i]; }
#pragma unroll
    for (int d = 0; d < D; ++d) { if (!valid) q[d] = 0.f; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const float p = expf(dot32(q, sK + j * D) * a.scale - l);
      acc[j] = MEAN ? acc[j] + p : p;
    }
  }
  if (!valid) return;
  float* pr = a.p + (int64_t)blockIdx.y * a.Lq * a.Lk + (int64_t)i * a.Lk;
  if (MEAN) {
#pragma unroll
    for (int j = 0; j < TQ; ++j) acc[j] *= a.inv_h;
  }
  if (a.Lk == 16) {
#pragma unroll
    for (int j = 0; j < TQ; j += 4) *reinterpret_cast<float4*>(pr + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < TQ; ++j)
      if (j < a.Lk) pr[j] = acc[j];
  }
}

int validate(const lmv_attn_desc* d, const float* p, int head_mean, int dtype) {
  if (!d) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: null descriptor");
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_DTYPE, "attn_probs: unsupported dtype %d", dtype);
  if (head_mean != 0 && head_mean != 1) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: head_mean must be 0 or 1, got %d", head_mean);
  if (d->B <= 0 || d->H <= 0 || d->Lq <= 0 || d->Lk <= 0) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: bad sizes B=%d H=%d Lq=%d Lk=%d", d->B, d->H, d->Lq, d->Lk);
  if (!(d->scale > 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: scale must be positive");
  if ((int64_t)d->Lq * d->Lk >= ((int64_t)1 << 31)) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: one (b, h) plane Lq * Lk = %d * %d must stay below 2^31", d->Lq, d->Lk);
  if ((int64_t)d->B * (head_mean ? 1 : d->H) > 65535 || (d->Lq + TQ - 1) / TQ > 65535)
    LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: at most 65535 output planes and 65535 * 16 queries per launch");
  const int64_t st[4] = {d->q_bs, d->q_rs, d->k_bs, d->k_rs};
  for (int i = 0; i < 4; ++i)
    if (st[i] % 8) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: strides must be multiples of 8 elements");
  if (!d->q || !d->k || !d->lse || !p) LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: null operand (q, k, lse and p are required)");
  if (!lmv_aligned16(d->q) || !lmv_aligned16(d->k) || !lmv_aligned16(p) || (((uintptr_t)d->lse) & 3u))
    LMV_FAIL(LMV_ERR_SHAPE, "attn_probs: misaligned operand (q, k, p: 16 bytes; lse: 4 bytes)");
  return LMV_OK;
}

template <bool MEAN>
void launch(const ProbArgs& a, int dtype, hipStream_t st) {
  const int planes = a.B * (MEAN ? 1 : a.H);
  if (a.Lk <= TQ) {
    const dim3 grid((a.Lq + QW - 1) / QW, planes);
    if (dtype == LMV_BF16) hipLaunchKernelGGL((probs_mfma_fewk_kernel<MEAN>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((probs_f32_fewk_kernel<MEAN>), grid, dim3(256), 0, st, a);
  } else {
    const dim3 grid((a.Lk + TK - 1) / TK, (a.Lq + TQ - 1) / TQ, planes);
    if (dtype == LMV_BF16) hipLaunchKernelGGL((probs_mfma_kernel<MEAN>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((probs_f32_kernel<MEAN>), grid, dim3(256), 0, st, a);
  }
}

}  // namespace

extern "C" int lmv_attn_probs(const lmv_attn_desc* d, float* p, int head_mean, int dtype, void* stream) {
  if (int rc = validate(d, p, head_mean, dtype)) return rc;
  ProbArgs a;
  a.q = d->q; a.k = d->k; a.lse = d->lse; a.p = p;
  a.q_bs = d->q_bs; a.q_rs = d->q_rs; a.k_bs = d->k_bs; a.k_rs = d->k_rs;
  a.B = d->B; a.H = d->H; a.Lq = d->Lq; a.Lk = d->Lk; a.scale = d->scale; a.inv_h = 1.f / (float)d->H;
  if (head_mean) launch<true>(a, dtype, (hipStream_t)stream);
  else launch<false>(a, dtype, (hipStream_t)stream);
  LMV_CHECK_LAUNCH("attn_probs");
  return LMV_OK;
}
