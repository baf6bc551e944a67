// convbn.hip -- training THROUGH a frozen (eval-mode) BatchNorm2d behind a 3 x 3 / stride-2 convolution (models/lemevit.py:698-704, :714-717; the reference's dense
// backbones keep every BatchNorm in eval mode): the BatchNorm is a per-channel affine map, so it is folded into the convolution's GEMM operand and never runs.
//
// (a) lmv_conv_bn_fold: ONE launch per convolution and pass.  With r = 1 / sqrt(var + eps), s = gamma r:
//       wm[co, col] = W[co, ci, tap] s[co]   (col = ci * 9 + tap: LMV_FOLD_CI_TAP, lmv_im2col3x3s2_c3 / _nchw;  col = tap * Cin + ci: LMV_FOLD_TAP_CI, lmv_im2col3x3s2_nhwc /
//                                             lmv_conv3x3s2_fwd), columns 9 Cin .. KP - 1 zero, in the compute type
//       bf[co] = (b[co] - mean[co]) s[co] + beta[co],   sc[co] = s[co]                       (fp32)
//     One thread per 16-byte chunk of wm; the thread of a row's first chunk writes the two vectors.
// (b) lmv_conv_bn_fold_bwd: ONE launch.  From the folded gradients dwm [Co, KP] / dbf [Co] of the weight-gradient GEMM (fp32):
//       dW[co, ci, tap] = dwm[co, col] s      db = dbf s      dgamma = r (sum_k dwm[co, k] W[co, k] + dbf (b - mean))      dbeta = dbf
//     written, not accumulated; each output may be NULL.  One workgroup per output channel; a thread sums columns tid, tid + 256, ... in that order and the 256
//     partial sums are combined by one fixed LDS tree: two launches agree bit for bit.
// (c) lmv_gelu_bwd_linear (behind lmv_linear_fwd(.., LMV_ACT_GELU_BWD)): out = aux * GELU'(a w^T + bias) -- the GELU backward of a convolution whose forward kept no
//     pre-activation: z is recomputed from the saved patch rows (K = 32 .. 288 on the image path: a patch row is not larger than a z row) and dz = da GELU'(z) leaves in
//     the same launch.  A kernel of its own (the epilogue of gemm_tiles.h is shared by the hot GEMMs of the train step, whose 4-wave forms sit on a 128-register budget):
//     a wave owns 16 rows and all N <= 128 columns; the weight tile is the MFMA "A" operand and the patch rows the "B" operand, so a lane ends up with four CONSECUTIVE
//     columns of one row (8 / 16-byte loads of aux, stores of out).  The weight matrix is staged in LDS once per workgroup where it fits in 64 KB.
#include <algorithm>
#include "common.h"

namespace {

constexpr int TPB = 256;

template <typename T>
__global__ __launch_bounds__(TPB) void fold_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ mean, const float* __restrict__ var, float eps, int Co, int Cin, int KP, int layout,
                                                   T* __restrict__ wm, float* __restrict__ bf, float* __restrict__ sc) {
  constexpr int EPC = DT<T>::EPC;
  const int cpr = KP / EPC, K = 9 * Cin;
  const int total = Co * cpr;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < total; i += gridDim.x * TPB) {
    const int co = i / cpr, j = i - co * cpr;
    const float s = gamma[co] * (1.0f / sqrtf(var[co] + eps));
    float v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int col = j * EPC + e;
      int src = col;                                             // LMV_FOLD_CI_TAP: the weight's own order
      if (layout == LMV_FOLD_TAP_CI) { const int tap = col / Cin, ci = col - tap * Cin; src = ci * 9 + tap; }
      v[e] = col < K ? w[(int64_t)co * K + src] * s : 0.f;
    }
    reinterpret_cast<uint4*>(wm)[i] = f_to_chunk<T>(v);
    if (j == 0) {
      bf[co] = ((b ? b[co] : 0.f) - mean[co]) * s + beta[co];
      sc[co] = s;
    }
  }
}

__global__ __launch_bounds__(TPB) void fold_bwd_kernel(const float* __restrict__ dwm, const float* __restrict__ dbf, const float* __restrict__ w, const float* __restrict__ b,
                                                       const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ var, float eps, int Cin, int KP,
                                                       int layout, float* __restrict__ dW, float* __restrict__ db, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[TPB];
  const int co = blockIdx.x, K = 9 * Cin;
  const float r = 1.0f / sqrtf(var[co] + eps), s = gamma[co] * r;
  float acc = 0.f;
  for (int k = threadIdx.x; k < K; k += TPB) {                   // k: the weight's own order ci * 9 + tap
    int col = k;
    if (layout == LMV_FOLD_TAP_CI) { const int ci = k / 9, tap = k - ci * 9; col = tap * Cin + ci; }
    const float g = dwm[(int64_t)co * KP + col];
    if (dW) dW[(int64_t)co * K + k] = g * s;
    acc += g * w[(int64_t)co * K + k];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int o = TPB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float g = dbf[co];
    if (db) db[co] = g * s;
    if (dgamma) dgamma[co] = r * (red[0] + g * ((b ? b[co] : 0.f) - mean[co]));
    if (dbeta) dbeta[co] = g;
  }
}

int fold_check(const char* who, int Co, int Cin, int KP, int layout) {
  if (Co <= 0 || Cin <= 0 || Cin > (1 << 16)) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape Co=%d Cin=%d", who, Co, Cin);
  if (Co % 8) LMV_FAIL(LMV_ERR_SHAPE, "%s: Co=%d must be a multiple of 8", who, Co);
  if (KP < 9 * Cin || (KP % 8)) LMV_FAIL(LMV_ERR_SHAPE, "%s: KP=%d must be a multiple of 8 and >= 9 Cin = %d", who, KP, 9 * Cin);
  if (layout != LMV_FOLD_CI_TAP && layout != LMV_FOLD_TAP_CI) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown layout %d", who, layout);
  if ((int64_t)Co * KP >= ((int64_t)1 << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: operand has >= 2^31 elements", who);
  return LMV_OK;
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c, bf16_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c, float) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}
template <typename T> __device__ __forceinline__ float gelu_grad_of(float x);
template <> __device__ __forceinline__ float gelu_grad_of<float>(float x) { return gelu_grad_f(x); }          // (the pair of the forward epilogue's GELU, gemm_tiles.h: act_gelu)
template <> __device__ __forceinline__ float gelu_grad_of<bf16_t>(float x) { return gelu_grad_fast_f(x); }

constexpr size_t GB_LDS_MAX = 64 * 1024;

// The K slot of a fragment element is the same permutation in both operands (lane group kq, k-step j, element e -> k = (4 j + kq) EPC + e), so 16-byte loads feed
// either MFMA form; a k-step covers 4 EPC columns.
template <typename T, int NT, bool STAGED>
__global__ __launch_bounds__(TPB) void gelu_bwd_kernel(const T* __restrict__ a, const T* __restrict__ w, const float* __restrict__ bias, const T* __restrict__ aux,
                                                      T* __restrict__ out, int M, int N, int K, int mtiles) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
  T* Ws = reinterpret_cast<T*>(gb_smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kq = lane >> 4;
  const int WST = K + 16 / (int)sizeof(T);                       // LDS row stride: 16 bytes of padding (rows of 16-byte chunks on distinct banks)
  const int cpr = K / EPC, ksteps = K / (4 * EPC);
  if (STAGED) {
    for (int i = threadIdx.x; i < N * cpr; i += TPB) {
      const int n = i / cpr, c = i - n * cpr;
      *reinterpret_cast<uint4*>(Ws + n * WST + c * EPC) = reinterpret_cast<const uint4*>(w)[i];
    }
    __syncthreads();
  }
  float4 b4[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = nt * 16 + 4 * kq;
    b4[nt] = (bias && n < N) ? *reinterpret_cast<const float4*>(bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int mt = blockIdx.x * 4 + wave; mt < mtiles; mt += gridDim.x * 4) {
    const int m = mt * 16 + r16;
    const T* arow = a + (int64_t)min(m, M - 1) * K;              // clamped address; rows behind M are never stored
    f32x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < ksteps; ++j) {
      const int k0 = (4 * j + kq) * EPC;
      const uint4 af = *reinterpret_cast<const uint4*>(arow + k0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + r16, nc = min(n, N - 1);
        uint4 wf = STAGED ? *reinterpret_cast<const uint4*>(Ws + nc * WST + k0) : *reinterpret_cast<const uint4*>(w + (int64_t)nc * K + k0);
        if (n >= N) wf = make_uint4(0, 0, 0, 0);
        acc[nt] = mma(wf, af, acc[nt], T());                     // C[n = 4 kq + e][m = r16]
      }
    }
    if (m < M) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + 4 * kq;
        if (n < N) {
          float g[4];
          ld4(aux + (int64_t)m * N + n, g);
          const float z[4] = {acc[nt][0] + b4[nt].x, acc[nt][1] + b4[nt].y, acc[nt][2] + b4[nt].z, acc[nt][3] + b4[nt].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] *= gelu_grad_of<T>(z[e]);
          st4(out + (int64_t)m * N + n, g);
        }
      }
    }
  }
}

template <typename T, int NT>
int launch_gelu_bwd(const lmv_linear_problem& q, int N, int K, hipStream_t st) {
  const int M = (int)q.rows, mtiles = (M + 15) / 16;
  const size_t lds = (size_t)N * (K * sizeof(T) + 16);
  const int grid = (int)std::min<int64_t>((mtiles + 3) / 4, 2048);
#define GB(STAGED, LDS) hipLaunchKernelGGL((gelu_bwd_kernel<T, NT, STAGED>), dim3(grid), dim3(TPB), LDS, st, (const T*)q.a, (const T*)q.w, q.bias, (const T*)q.aux, (T*)q.out, M, N, K, mtiles)
  if (lds <= GB_LDS_MAX) GB(true, lds); else GB(false, 0);
#undef GB
  return LMV_OK;
}

template <typename T>
int launch_gelu_bwd_nt(const lmv_linear_problem& q, int N, int K, hipStream_t st) {
  const int nt = (N + 15) / 16;
  if (nt <= 2) return launch_gelu_bwd<T, 2>(q, N, K, st);
  if (nt <= 4) return launch_gelu_bwd<T, 4>(q, N, K, st);
  if (nt <= 6) return launch_gelu_bwd<T, 6>(q, N, K, st);
  return launch_gelu_bwd<T, 8>(q, N, K, st);
}

}  // namespace

int lmv_gelu_bwd_linear(const lmv_linear_problem* p, int nproblems, int N, int K, int dtype, hipStream_t st) {
  if (nproblems < 1 || nproblems > 2 || !p) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): nproblems must be 1 or 2 (got %d)", nproblems);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_DTYPE, "linear_fwd(GELU_BWD): unsupported dtype %d", dtype);
  if (N <= 0 || K <= 0 || (N % 8) || (K % 32) || N > 128) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): N=%d must be a multiple of 8, at most 128, K=%d a multiple of 32", N, K);
  for (int i = 0; i < nproblems; ++i) {
    const lmv_linear_problem& q = p[i];
    if (!q.aux) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): aux (the incoming gradient [rows, N]) is required");
    if (q.res || q.row_scale || q.out_pre) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): takes no residual, row scale or pre-activation copy");
    if (q.rows <= 0 || q.rows > 0x7fffffffLL / 16) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): bad rows %lld", (long long)q.rows);
    if (!q.a || !q.w || !q.out) LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): null operand");
    if (!lmv_aligned16(q.a) || !lmv_aligned16(q.w) || !lmv_aligned16(q.out) || !lmv_aligned16(q.aux) || !lmv_aligned16(q.bias))
      LMV_FAIL(LMV_ERR_SHAPE, "linear_fwd(GELU_BWD): operands must be 16-byte aligned");
  }
  for (int i = 0; i < nproblems; ++i) {
    if (dtype == LMV_BF16) launch_gelu_bwd_nt<bf16_t>(p[i], N, K, st); else launch_gelu_bwd_nt<float>(p[i], N, K, st);
  }
  LMV_CHECK_LAUNCH("linear_fwd(GELU_BWD)");
  return LMV_OK;
}

extern "C" int lmv_conv_bn_fold(const float* w, const float* b, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int Co, int Cin, int KP,
                                int layout, void* wm, float* bf, float* sc, int dtype, void* stream) {
  if (int rc = fold_check("conv_bn_fold", Co, Cin, KP, layout)) return rc;
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_DTYPE, "conv_bn_fold: unsupported dtype %d", dtype);
  if (!w || !gamma || !beta || !mean || !var || !wm || !bf || !sc) LMV_FAIL(LMV_ERR_SHAPE, "conv_bn_fold: null operand");
  if (!lmv_aligned16(wm)) LMV_FAIL(LMV_ERR_SHAPE, "conv_bn_fold: misaligned operand matrix");
  if (!(eps >= 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "conv_bn_fold: eps must be >= 0");
  const int total = Co * (KP / (dtype == LMV_BF16 ? 8 : 4));
  const dim3 grid((total + TPB - 1) / TPB), block(TPB);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LMV_BF16) hipLaunchKernelGGL((fold_kernel<bf16_t>), grid, block, 0, st, w, b, gamma, beta, mean, var, eps, Co, Cin, KP, layout, (bf16_t*)wm, bf, sc);
  else hipLaunchKernelGGL((fold_kernel<float>), grid, block, 0, st, w, b, gamma, beta, mean, var, eps, Co, Cin, KP, layout, (float*)wm, bf, sc);
  LMV_CHECK_LAUNCH("conv_bn_fold");
  return LMV_OK;
}

extern "C" int lmv_conv_bn_fold_bwd(const float* dwm, const float* dbf, const float* w, const float* b, const float* gamma, const float* mean, const float* var, float eps,
                                    int Co, int Cin, int KP, int layout, float* dW, float* db, float* dgamma, float* dbeta, void* stream) {
  if (int rc = fold_check("conv_bn_fold_bwd", Co, Cin, KP, layout)) return rc;
  if (!dwm || !dbf || !w || !gamma || !mean || !var) LMV_FAIL(LMV_ERR_SHAPE, "conv_bn_fold_bwd: null operand");
  if (!(eps >= 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "conv_bn_fold_bwd: eps must be >= 0");
  if (!dW && !db && !dgamma && !dbeta) return LMV_OK;
  hipLaunchKernelGGL(fold_bwd_kernel, dim3(Co), dim3(TPB), 0, (hipStream_t)stream, dwm, dbf, w, b, gamma, mean, var, eps, Cin, KP, layout, dW, db, dgamma, dbeta);
  LMV_CHECK_LAUNCH("conv_bn_fold_bwd");
  return LMV_OK;
}
