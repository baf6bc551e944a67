// dense.hip -- the losses and metrics behind a dense-prediction head (the reference's change_detection/utils/metrics.py FocalLoss / dice_loss / jaccard_loss and
// utils/losses.py hybrid_loss, train.py:154-260, eval.py:39-66; the segmentation heads' per-pixel cross-entropy with an ignore index and the mIoU histogram):
//   lmv_dense_loss_fwd: (a) ONE pass over NCHW logits and a label map -> per workgroup one row of fp32 partial sums (P_k, I_k, T_k, the weighted and the plain
//                       negative log-likelihood, the valid count), optionally the argmax map and the confusion counts; (b) ONE workgroup adds the rows in double
//                       and writes the `stats` vector (losses, 1 / D and the gradient table u_k, v_k);
//   lmv_dense_loss_bwd: ONE pass that re-reads logits and labels and writes every element of dlogits once from that table.
//   lmv_dense_up_loss_fwd / _bwd: the same on bilinearly upsampled low-resolution logits, interpolated inside the pass;
//   lmv_dense_slide_fwd: the forward pass on the mean of overlapping windows' upsampled logits (sliding-window inference: stitch, resize and argmax in one pass).
// A pixel's classes are K planes a whole image apart: a thread owns a CHUNK of 16 bytes of consecutive pixels (4 fp32 / 8 bf16) and reads one 16-byte word per class
// plane where base and strides allow, element loads otherwise.  The chunks, the arithmetic behind the loads and every summation order are the same on both paths.
// No floating-point atomics: per-thread partials, a butterfly per wave, waves in order, rows in order.  Counts that go through atomics are integers.
#include <math.h>
#include <algorithm>
#include <type_traits>
#include "common.h"

// one expression must give one value wherever the compiler places it (the vector and the element path share the code behind the loads)
#pragma clang fp contract(off)

namespace {
constexpr int DN_MAX_WG = 1024;          // workgroups of the forward pass: more chunks than DN_MAX_WG * threads are taken in further sweeps of the grid-stride loop
constexpr int DN_MAX_WG_BWD = 2048;
constexpr int DN_KREG = 5;               // K <= DN_KREG: class values and partial sums in registers; above: values re-read from cache, partial sums in LDS

// what every kernel here is told, whatever the resolution of the logits.  dn_head fills the inputs; the entry points add the buffers of their direction
// (ws / pred / conf, or stats / gout / dlogits) and dn_args / up_args the chunk count.
struct DenseHead {
  const void* logits; const void* labels; const float* alpha;
  float* ws; uint8_t* pred; unsigned long long* conf;
  const float* stats; const float* gout; void* dlogits;
  int64_t sb, sc, ignore, nchunks;
  int B, K;
};
// The loss terms the kernels need.  A member BEHIND the sizes of either argument struct, not part of the head: dense_up_bwd_kernel sits at the SGPR limit, and
// with these three in front of its sizes the kernel-argument loads regroup and it spills more scalars (profiles/dense_refactor_resources.txt).
struct DenseTerms {
  float gamma, w_ce;
  int shape_terms;          // w_dice or w_jac is not 0: the u / v table matters
};
struct DenseArgs : DenseHead {
  int HW, cpi;          // cpi: chunks per image
  int xvec, lvec, pvec, dvec;          // 16-byte logits loads / vector label loads / vector pred stores / 16-byte dlogits stores are possible for FULL chunks
  DenseTerms t;
};

static inline int dn_threads(int K) { return K <= 16 ? 256 : (K <= 32 ? 128 : 64); }          // K > DN_KREG: 2 K threads floats of LDS stay at 32 KB
static inline int64_t dn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T> __device__ __forceinline__ void dn_load(const T* p, bool vec, int n, float* f) {
  constexpr int V = DT<T>::EPC;
  if (vec) {
    const uint4 c = *reinterpret_cast<const uint4*>(p);
    chunk_to_f<T>(c, f);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = j < n ? DT<T>::ld(p + j) : 0.f;
  }
}

template <typename T> __device__ __forceinline__ void dn_store(T* p, bool vec, int n, const float* f) {
  constexpr int V = DT<T>::EPC;
  if (vec) {
    *reinterpret_cast<uint4*>(p) = f_to_chunk<T>(f);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < n) DT<T>::st(p + j, f[j]);
  }
}

// labels of a chunk -> class index, or -1 for an ignored pixel (label == ignore, outside [0, K), or behind the end of the image)
template <int V> __device__ __forceinline__ void dn_labels(const int64_t* p, bool vec, int n, int64_t ignore, int K, int* y) {
  int64_t v[V];
  if (vec) {
#pragma unroll
    for (int j = 0; j < V / 2; ++j) { const longlong2 w = reinterpret_cast<const longlong2*>(p)[j]; v[2 * j] = w.x; v[2 * j + 1] = w.y; }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = j < n ? p[j] : (int64_t)-1;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) y[j] = (v[j] >= 0 && v[j] < K && v[j] != ignore) ? (int)v[j] : -1;
}
template <int V> __device__ __forceinline__ void dn_labels(const uint8_t* p, bool vec, int n, int64_t ignore, int K, int* y) {
  int v[V];
  if (vec) {
    if (V == 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = (int)((w >> (8 * j)) & 255u);
    } else {
      const uint2 w = *reinterpret_cast<const uint2*>(p);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = (int)(((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 255u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = j < n ? (int)p[j] : -1;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) y[j] = (v[j] >= 0 && v[j] < K && (int64_t)v[j] != ignore) ? v[j] : -1;
}

// the argmax rule: a later class replaces the best only when it is greater, or a NaN while the best is a number (-0 == +0 compare equal: the first stays)
__device__ __forceinline__ bool dn_better(float v, float best) { return v > best || (v != v && best == best); }

__device__ __forceinline__ float dn_focal(const float* alpha, float gamma, int y, float py) {
  float f = alpha ? alpha[y] : 1.f;
  if (gamma > 0.f) f = f * expf(gamma * logf(fmaxf(1.f - py, 0.f)));          // (1 - p_y)^gamma; 1 - p_y == 0: exp(-inf) = 0
  return f;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the pieces that the native and the upsampling kernels share: each rule of the loss is stated here once ----
// The forward LDS (dynamic), one layout for both forward kernels:
//   KT > 0: red [waves][3 KT + 3] floats | conf [K K] ints;  KT == 0: accP [K][threads] | accI [K][threads] floats | cntT [K] ints | red [waves][3] | conf
struct DnLds { float* accP; float* accI; int* cntT; float* red; int* conf; };
static inline size_t dn_lds_bytes(int K, int NT, bool has_conf, int kreg = DN_KREG) {          // kreg: the largest K of the launched kernel's register instances
  const size_t nw = NT / 64;
  return (K <= kreg ? nw * (3 * K + 3) : (size_t)2 * K * NT + K + nw * 3) * sizeof(float) + (has_conf ? (size_t)K * K * sizeof(int) : 0);
}
// sums: the pass accumulates (the upsampling kernel's prediction-only form does not: nothing to zero, no barrier)
template <int KT> __device__ __forceinline__ DnLds dn_lds(float* smem, int K, bool sums, bool has_conf) {
  const int NT = blockDim.x, tid = threadIdx.x, nw = NT >> 6;
  DnLds s;
  s.accP = smem;
  s.accI = smem + (KT > 0 ? 0 : K * NT);
  s.cntT = reinterpret_cast<int*>(smem + (KT > 0 ? 0 : 2 * K * NT));
  s.red = smem + (KT > 0 ? 0 : 2 * K * NT + K);
  s.conf = reinterpret_cast<int*>(s.red + nw * (KT > 0 ? 3 * KT + 3 : 3));
  if (sums) {
    if (KT == 0) {
      for (int i = tid; i < 2 * K * NT; i += NT) smem[i] = 0.f;
      for (int i = tid; i < K; i += NT) s.cntT[i] = 0;
    }
    if (has_conf)
      for (int i = tid; i < K * K; i += NT) s.conf[i] = 0;
    __syncthreads();
  }
  return s;
}

// The register path's pixel (KT > 0), stated once for both forward kernels.  Z(k): the lvalue of the pixel's k-th logit, reused for the exponentials (no second
// set of registers).  Leaves the argmax, sum exp(z - max), z_y - max and p_y in bi, se, zy, py and adds the pixel to the thread's partial sums rP, rI, rT.  An
// ignored pixel (y < 0) contributes to nothing; SKIP (a constant at both sites, which say why): its softmax is branched around, not evaluated and discarded.
// A macro and not a __forceinline__ function: as a function, in every form tried (pointers, references, a struct returned by value), the compiler turns the
// conditional updates of dense_fwd_kernel into selects, whose lane masks cost that kernel about 20 scalar registers and, for fp32 logits with int64 labels
// at K = 2, 3, a wave of occupancy.  The text below compiles to the registers the kernels had (profiles/dense_refactor_resources.txt).
#define DN_PIXEL(KT, Z, y, SKIP, bi, se, zy, py, rP, rI, rT)                      \
  do {                                                                            \
    float best_ = Z(0), m_ = Z(0);                                                \
    int b_ = 0;                                                                   \
    _Pragma("unroll") for (int k = 1; k < KT; ++k) {                              \
      if (dn_better(Z(k), best_)) { best_ = Z(k); b_ = k; }                       \
      m_ = fmaxf(m_, Z(k));                                                       \
    }                                                                             \
    bi = b_; se = 1.f; zy = 0.f; py = 0.f;                                        \
    const bool on_ = (y) >= 0;                                                    \
    if (on_ || !(SKIP)) {                                                         \
      float s_ = 0.f;                                                             \
      _Pragma("unroll") for (int k = 0; k < KT; ++k) {                            \
        const float dz_ = Z(k) - m_;                                              \
        if ((y) == k) zy = dz_;          /* z_y - max */                          \
        Z(k) = expf(dz_); s_ += Z(k);                                             \
      }                                                                           \
      se = s_;                                                                    \
      const float inv_ = 1.f / s_;                                                \
      _Pragma("unroll") for (int k = 0; k < KT; ++k) {                            \
        const float p_ = Z(k) * inv_;                                             \
        if (on_) rP[k] += p_;                                                     \
        if ((y) == k) { rI[k] += p_; rT[k] += 1; py = p_; }                       \
      }                                                                           \
    }                                                                             \
  } while (0)

// the tail of a pixel on either path: its negative log-likelihood, plain and focal-weighted, the valid count and the workgroup's confusion counts in LDS
__device__ __forceinline__ void dn_pixel_tail(const DenseHead& a, const DenseTerms& t, int K, int* conf, int y, int bi, float se, float zy, float py, float& ce_sum, float& nll_sum,
                                              int& nvalid) {
  if (y >= 0) {
    const float nll = logf(se) - zy;          // -log p_y = log(sum exp(z - max)) - (z_y - max)
    ce_sum += dn_focal(a.alpha, t.gamma, y, py) * nll;
    nll_sum += nll;
    nvalid += 1;
    if (a.conf) atomicAdd(&conf[y * K + bi], 1);
  }
}

// the argmax of a chunk's V pixels: one 32-bit / 64-bit word where the caller found pp aligned and the chunk whole, bytes otherwise
template <int V> __device__ __forceinline__ void dn_store_pred(uint8_t* pp, bool vec, int n, const int* bi) {
  if (vec) {
    uint32_t w[V / 4] = {};
#pragma unroll
    for (int j = 0; j < V; ++j) w[j >> 2] |= (uint32_t)bi[j] << (8 * (j & 3));
    if constexpr (V == 4) *reinterpret_cast<uint32_t*>(pp) = w[0];
    else *reinterpret_cast<uint2*>(pp) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < n) pp[j] = (uint8_t)bi[j];
  }
}

// The gradient of a valid pixel's class k from the u / v table: g = cf (p - [hit]) + p ((v + [hit] u) - sg).  p, sg = sum_k p_k (v_k + [hit] u_k) and the CE
// factor cf are the caller's: the two backward passes form p and sg in different orders (see dense_up_bwd_kernel), and those bits stay as they are.
// dn_grad reads the table row through pointers, inside the branch (dense_bwd_kernel's register form pays VGPRs for loads hoisted out of it), and writes
// dn_shape's expression out: with the call nested here dense_up_bwd_kernel, which sits at the SGPR limit, spills more scalars.
__device__ __forceinline__ float dn_shape(bool hit, float uk, float vk) { return vk + (hit ? uk : 0.f); }
__device__ __forceinline__ float dn_cf(const DenseHead& a, const DenseTerms& t, float invD, int y, float py) { return t.w_ce * dn_focal(a.alpha, t.gamma, y, py) * invD; }
__device__ __forceinline__ float dn_grad(const DenseTerms& t, float p, bool hit, float cf, const float* U, const float* Vt, int k, float sg, float gout) {
  float g = cf * (p - (hit ? 1.f : 0.f));
  if (t.shape_terms) g = p * ((Vt[k] + (hit ? U[k] : 0.f)) - sg) + g;
  return gout * g;
}

// chunk -> image, offsets and length
struct DnChunk { int64_t xoff, poff, doff; int n; };          // element offsets into the logits, into labels / pred, into dlogits (class 0)
__device__ __forceinline__ DnChunk dn_chunk(const DenseArgs& a, int64_t ch, int V) {
  const int b = (int)(ch / a.cpi);
  const int p0 = (int)(ch - (int64_t)b * a.cpi) * V;
  DnChunk c;
  c.xoff = (int64_t)b * a.sb + p0;
  c.poff = (int64_t)b * a.HW + p0;
  c.doff = (int64_t)b * a.K * a.HW + p0;
  c.n = min(V, a.HW - p0);
  return c;
}

// ---- the workgroup's row: butterfly per wave, waves in order (the tail of both forward kernels) ----
template <int KT> __device__ __forceinline__ void dn_write_row(float* ws, unsigned long long* gconf, int K, float* smem, float* red, const int* cntT, const int* conf,
                                                               const float* rP, const float* rI, const int* rT, float ce_sum, float nll_sum, int nvalid) {
  const int NT = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  float* row = ws + (int64_t)blockIdx.x * (3 * K + 3);
  ce_sum = wave_sum(ce_sum); nll_sum = wave_sum(nll_sum); nvalid = wave_sum_int(nvalid);
  if constexpr (KT > 0) {
    constexpr int NA = 3 * KT + 3;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const float p = wave_sum(rP[k]), i = wave_sum(rI[k]);
      const int t = wave_sum_int(rT[k]);
      if (lane == 0) { red[wave * NA + k] = p; red[wave * NA + KT + k] = i; red[wave * NA + 2 * KT + k] = (float)t; }
    }
    if (lane == 0) { red[wave * NA + 3 * KT] = ce_sum; red[wave * NA + 3 * KT + 1] = nll_sum; red[wave * NA + 3 * KT + 2] = (float)nvalid; }
    __syncthreads();
    if (tid < NA) {
      float s = red[tid];
      for (int w = 1; w < nw; ++w) s += red[w * NA + tid];
      row[tid] = s;
    }
  } else {
    if (lane == 0) { red[wave * 3] = ce_sum; red[wave * 3 + 1] = nll_sum; red[wave * 3 + 2] = (float)nvalid; }
    __syncthreads();
    for (int col = wave; col < 2 * K; col += nw) {          // accP | accI are one [2 K][threads] array
      float s = smem[col * NT + lane];
      for (int i = 64; i < NT; i += 64) s += smem[col * NT + lane + i];
      s = wave_sum(s);
      if (lane == 0) row[col] = s;
    }
    for (int k = tid; k < K; k += NT) row[2 * K + k] = (float)cntT[k];
    if (tid < 3) {
      float s = red[tid];
      for (int w = 1; w < nw; ++w) s += red[w * 3 + tid];
      row[3 * K + tid] = s;
    }
  }
  if (gconf) {          // (after a __syncthreads on either path) integer adds commute: the matrix does not depend on their order
    for (int i = tid; i < K * K; i += NT) {
      const int cnt = conf[i];
      if (cnt) atomicAdd(&gconf[i], (unsigned long long)cnt);
    }
  }
}

// ---- (a) the forward pass ---------------------------------------------------------------------------------------------------------------------------
template <typename T, typename LT, int KT> __global__ __launch_bounds__(256) void dense_fwd_kernel(const DenseArgs a) {
  constexpr int V = DT<T>::EPC;
  constexpr int KR = KT > 0 ? KT : 1;
  extern __shared__ float smem[];
  const int K = KT > 0 ? KT : a.K;
  const int NT = blockDim.x, tid = threadIdx.x;
  const DnLds s = dn_lds<KT>(smem, K, true, a.conf != nullptr);
  float* accP = s.accP;
  float* accI = s.accI;

  float rP[KR], rI[KR];
  int rT[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) { rP[k] = 0.f; rI[k] = 0.f; rT[k] = 0; }
  float ce_sum = 0.f, nll_sum = 0.f;
  int nvalid = 0;
  const T* X = reinterpret_cast<const T*>(a.logits);
  const LT* L = reinterpret_cast<const LT*>(a.labels);

  for (int64_t ch = (int64_t)blockIdx.x * NT + tid; ch < a.nchunks; ch += (int64_t)gridDim.x * NT) {
    const DnChunk c = dn_chunk(a, ch, V);
    const bool full = c.n == V;
    const T* x = X + c.xoff;
    int y[V];
    dn_labels<V>(L + c.poff, a.lvec && full, c.n, a.ignore, K, y);
    float se[V], zy[V], py[V];
    int bi[V];
    if constexpr (KT > 0) {
      float z[KT][V];
#pragma unroll
      for (int k = 0; k < KT; ++k) dn_load<T>(x + k * a.sc, a.xvec && full, c.n, z[k]);
      // column j of z.  Ignored pixels are NOT branched around here: V branches per chunk cost this pass scalar registers and, at K = 3, a wave of occupancy
#define DN_Z(k) z[k][j]
#pragma unroll
      for (int j = 0; j < V; ++j) DN_PIXEL(KT, DN_Z, y[j], false, bi[j], se[j], zy[j], py[j], rP, rI, rT);
#undef DN_Z
    } else {
      // DELIBERATELY not the upsampling kernel's generic path: class-major over the chunk, ONE 16-byte load per class plane for V pixels (this pass is the
      // memory-bound one), and the softmax of an ignored pixel is evaluated and discarded rather than branched around
      float f[V], mx[V];
      dn_load<T>(x, a.xvec && full, c.n, f);
#pragma unroll
      for (int j = 0; j < V; ++j) { mx[j] = f[j]; se[j] = f[j]; bi[j] = 0; }          // se: the best value so far
      for (int k = 1; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (dn_better(f[j], se[j])) { se[j] = f[j]; bi[j] = k; }
          mx[j] = fmaxf(mx[j], f[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) se[j] = 0.f;
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
#pragma unroll
        for (int j = 0; j < V; ++j) se[j] += expf(f[j] - mx[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) { zy[j] = 0.f; py[j] = 0.f; }
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
        float sp = accP[k * NT + tid];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float e = expf(f[j] - mx[j]);
          const float p = e * (1.f / se[j]);
          if (y[j] >= 0) sp += p;
          if (y[j] == k) { accI[k * NT + tid] += p; atomicAdd(&s.cntT[k], 1); zy[j] = f[j] - mx[j]; py[j] = p; }
        }
        accP[k * NT + tid] = sp;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) dn_pixel_tail(a, a.t, K, s.conf, y[j], bi[j], se[j], zy[j], py[j], ce_sum, nll_sum, nvalid);
    if (a.pred) dn_store_pred<V>(a.pred + c.poff, a.pvec && full, c.n, bi);
  }

  dn_write_row<KT>(a.ws, a.conf, K, smem, s.red, s.cntT, s.conf, rP, rI, rT, ce_sum, nll_sum, nvalid);
}

// ---- (b) rows -> stats ------------------------------------------------------------------------------------------------------------------------------
struct DenseFinArgs {
  const float* ws; const float* alpha; float* stats; double* meter;
  int rows, K, avg_mode;
  double npix, w_ce, w_dice, w_jac, eps;
};

__device__ __forceinline__ double dn_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ONE workgroup of four waves.  Column j of the rows: wave j % 4, lane l adds rows l, l + 64, ... in order, then the butterfly, all in double.  Then thread k forms
// class k's terms and thread 0 adds them in class order.
__global__ __launch_bounds__(256) void dense_finalize_kernel(const DenseFinArgs a) {
  __shared__ double col[3 * LMV_DENSE_MAX_CLASSES + 3];
  __shared__ double term[3][LMV_DENSE_MAX_CLASSES];
  const int K = a.K, ncol = 3 * K + 3, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = wave; j < ncol; j += 4) {
    double s = 0.0;
    for (int r = lane; r < a.rows; r += 64) s += (double)a.ws[(int64_t)r * ncol + j];
    s = dn_wave_sum_f64(s);
    if (lane == 0) col[j] = s;
  }
  __syncthreads();
  float* st = a.stats;
  if (tid < K) {
    const double P = col[tid], I = col[K + tid], Tk = col[2 * K + tid];
    const double C = P + Tk + a.eps, U = P + Tk - I + a.eps;
    term[0][tid] = 2.0 * I / C;
    term[1][tid] = I / U;
    term[2][tid] = (a.alpha ? (double)a.alpha[tid] : 1.0) * Tk;
    st[LMV_DENSE_STATS_HEAD + tid] = (float)(-a.w_dice * 2.0 / (K * C) - a.w_jac * (1.0 / U + I / (U * U)) / K);          // u_k
    st[LMV_DENSE_STATS_HEAD + K + tid] = (float)(a.w_dice * 2.0 * I / (K * C * C) + a.w_jac * I / (K * U * U));          // v_k
    st[LMV_DENSE_STATS_HEAD + 2 * K + tid] = (float)I;
    st[LMV_DENSE_STATS_HEAD + 3 * K + tid] = (float)P;
    st[LMV_DENSE_STATS_HEAD + 4 * K + tid] = (float)Tk;
  }
  __syncthreads();
  if (tid == 0) {
    double sd = 0.0, sj = 0.0, sw = 0.0;
    for (int k = 0; k < K; ++k) { sd += term[0][k]; sj += term[1][k]; sw += term[2][k]; }
    const double nvalid = col[3 * K + 2];
    const double D = a.avg_mode == LMV_DENSE_AVG_VALID ? nvalid : (a.avg_mode == LMV_DENSE_AVG_ALL ? a.npix : sw);
    const double invD = D > 0.0 ? 1.0 / D : 0.0;
    const double ce = col[3 * K] * invD, dice = 1.0 - sd / K, jac = 1.0 - sj / K;
    st[0] = (float)(a.w_ce * ce + a.w_dice * dice + a.w_jac * jac);
    st[1] = (float)ce; st[2] = (float)dice; st[3] = (float)jac; st[4] = (float)nvalid; st[5] = (float)invD;
    if (a.meter) { a.meter[0] += col[3 * K + 1]; a.meter[1] += nvalid; }          // stream order serialises successive updates
  }
}

// ---- the backward pass ------------------------------------------------------------------------------------------------------------------------------
template <typename T, typename LT, int KT> __global__ __launch_bounds__(256) void dense_bwd_kernel(const DenseArgs a) {
  constexpr int V = DT<T>::EPC;
  const int K = KT > 0 ? KT : a.K;
  const int NT = blockDim.x;
  const T* X = reinterpret_cast<const T*>(a.logits);
  const LT* L = reinterpret_cast<const LT*>(a.labels);
  T* DL = reinterpret_cast<T*>(a.dlogits);
  const float gout = a.gout ? *a.gout : 1.f;
  const float invD = a.stats[5];
  const float* U = a.stats + LMV_DENSE_STATS_HEAD;
  const float* Vt = U + K;
  const int64_t plane = a.HW;
  for (int64_t ch = (int64_t)blockIdx.x * NT + threadIdx.x; ch < a.nchunks; ch += (int64_t)gridDim.x * NT) {
    const DnChunk c = dn_chunk(a, ch, V);
    const bool full = c.n == V;
    const T* x = X + c.xoff;
    T* d = DL + c.doff;
    int y[V];
    dn_labels<V>(L + c.poff, a.lvec && full, c.n, a.ignore, K, y);
    if constexpr (KT > 0) {
      float z[KT][V];
#pragma unroll
      for (int k = 0; k < KT; ++k) dn_load<T>(x + k * a.sc, a.xvec && full, c.n, z[k]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float m = z[0][j];
#pragma unroll
        for (int k = 1; k < KT; ++k) m = fmaxf(m, z[k][j]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) { z[k][j] = expf(z[k][j] - m); s += z[k][j]; }
        const float inv = 1.f / s;
        float py = 0.f, sg = 0.f;          // sg = sum_k p_k (v_k + [hit] u_k) with p_k = e_k inv: NOT the upsampling backward's (sum_k e_k (..)) inv
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          z[k][j] = z[k][j] * inv;          // p_k
          const bool hit = y[j] == k;
          if (hit) py = z[k][j];
          if (a.t.shape_terms) sg += z[k][j] * dn_shape(hit, U[k], Vt[k]);
        }
        const bool on = y[j] >= 0;
        const float cf = on ? dn_cf(a, a.t, invD, y[j], py) : 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) z[k][j] = on ? dn_grad(a.t, z[k][j], y[j] == k, cf, U, Vt, k, sg, gout) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) dn_store<T>(d + k * plane, a.dvec && full, c.n, z[k]);
    } else {
      float f[V], mx[V], se[V], sg[V], py[V], cf[V];
      dn_load<T>(x, a.xvec && full, c.n, f);
#pragma unroll
      for (int j = 0; j < V; ++j) mx[j] = f[j];
      for (int k = 1; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
#pragma unroll
        for (int j = 0; j < V; ++j) mx[j] = fmaxf(mx[j], f[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) { se[j] = 0.f; sg[j] = 0.f; py[j] = 0.f; }
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
#pragma unroll
        for (int j = 0; j < V; ++j) se[j] += expf(f[j] - mx[j]);
      }
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
        const float uk = U[k], vk = Vt[k];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float p = expf(f[j] - mx[j]) * (1.f / se[j]);
          const bool hit = y[j] == k;
          if (hit) py[j] = p;
          if (a.t.shape_terms) sg[j] += p * dn_shape(hit, uk, vk);
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) cf[j] = y[j] >= 0 ? dn_cf(a, a.t, invD, y[j], py[j]) : 0.f;
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float p = expf(f[j] - mx[j]) * (1.f / se[j]);
          f[j] = y[j] >= 0 ? dn_grad(a.t, p, y[j] == k, cf[j], U, Vt, k, sg[j], gout) : 0.f;
        }
        dn_store<T>(d + k * plane, a.dvec && full, c.n, f);
      }
    }
  }
}

// ---- the same losses on bilinearly upsampled logits -------------------------------------------------------------------------------------------------
// logits [B, K, h, w] -> PyTorch's upsample_bilinear2d to the label map's [H, W] (the `size=` form: the scale comes from the sizes), evaluated per output pixel in
// fp32 and never stored.  A bf16 input is NOT rounded back to bf16 after the interpolation (the stock path rounds the [B, K, H, W] map it writes): more accurate.
struct UpArgs : DenseHead {
  int h, w, H, W, cpr, align;          // cpr: chunks per output row
  float sy, sx;          // input / output (align_corners: (in - 1) / (out - 1), 0 when out == 1), in float as PyTorch computes it
  DenseTerms t;
  int TH, TW, FBH, FBW, tiles_y, tiles_x, G;          // backward: the tile of input pixels, the block of output pixels in LDS, threads per input pixel of the gather
};

constexpr int UP_V = 4;          // output pixels of a chunk (both dtypes: the labels of a chunk are one 32-bit / two 16-byte words, its pred one 32-bit word)
constexpr int UP_FB = 40;          // the backward's block of output pixels is at most UP_FB x UP_FB

// THE index function of every kernel here: output coordinate -> the two taps and the weight of the second.  i0 is non-decreasing in dst (a product with a positive
// constant, rounded), which is what up_first / up_end rely on.
struct UpAxis { int i0, i1; float l; };
__device__ __forceinline__ UpAxis up_axis(int dst, int in, float scale, int align) {
  const float src = align ? (float)dst * scale : fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.f);
  UpAxis a;
  a.i0 = min((int)src, in - 1);
  a.i1 = min(a.i0 + 1, in - 1);
  a.l = src - (float)a.i0;
  return a;
}
// the weight of input index i in the output coordinate behind ax (both taps on one index at the clamped border: both count, as in the forward pass)
__device__ __forceinline__ float up_weight(int i0, int i1, float l, int i) { return (i == i0 ? 1.f - l : 0.f) + (i == i1 ? l : 0.f); }
// the output coordinates that touch input indices [t0, t1]: [up_first(t0), up_end(t1)), found by bisection on up_axis itself -- no inverse map, nothing to round
__device__ __forceinline__ int up_first(int t, int in, int out, float scale, int align) {
  int lo = 0, hi = out;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (up_axis(mid, in, scale, align).i1 >= t) hi = mid; else lo = mid + 1; }
  return lo;
}
__device__ __forceinline__ int up_end(int t, int in, int out, float scale, int align) {
  int lo = 0, hi = out;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (up_axis(mid, in, scale, align).i0 > t) hi = mid; else lo = mid + 1; }
  return lo;
}
// one class plane at one output pixel: r0 / r1 are the row offsets of the two input rows
template <typename T> __device__ __forceinline__ float up_tap(const T* p, int r0, int r1, int c0, int c1, float ly, float lx) {
  const float z00 = DT<T>::ld(p + r0 + c0), z01 = DT<T>::ld(p + r0 + c1), z10 = DT<T>::ld(p + r1 + c0), z11 = DT<T>::ld(p + r1 + c1);
  return (1.f - ly) * ((1.f - lx) * z00 + lx * z01) + ly * ((1.f - lx) * z10 + lx * z11);
}

// ---- forward: a thread owns chunks of UP_V consecutive output pixels of ONE output row; the LDS layout, the pixel, the row and the summation discipline of dense_fwd_kernel ----
// labels == NULL: prediction only (argmax map, no sums, no row).
template <typename T, typename LT, int KT> __global__ __launch_bounds__(256) void dense_up_fwd_kernel(const UpArgs a) {
  constexpr int V = UP_V;
  constexpr int KR = KT > 0 ? KT : 1;
  extern __shared__ float smem[];
  const int K = KT > 0 ? KT : a.K;
  const int NT = blockDim.x, tid = threadIdx.x;
  const bool sums = a.labels != nullptr;
  const DnLds s = dn_lds<KT>(smem, K, sums, a.conf != nullptr);
  float rP[KR], rI[KR];
  int rT[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) { rP[k] = 0.f; rI[k] = 0.f; rT[k] = 0; }
  float ce_sum = 0.f, nll_sum = 0.f;
  int nvalid = 0;
  const T* X = reinterpret_cast<const T*>(a.logits);
  const LT* L = reinterpret_cast<const LT*>(a.labels);

  for (int64_t ch = (int64_t)blockIdx.x * NT + tid; ch < a.nchunks; ch += (int64_t)gridDim.x * NT) {
    const int64_t orow = ch / a.cpr;          // b H + Y
    const int X0 = (int)(ch - orow * a.cpr) * V;
    const int b = (int)(orow / a.H), Y = (int)(orow - (int64_t)b * a.H);
    const int n = min(V, a.W - X0);
    const int64_t poff = orow * a.W + X0;
    const T* x = X + (int64_t)b * a.sb;
    const UpAxis ay = up_axis(Y, a.h, a.sy, a.align);
    const int r0 = ay.i0 * a.w, r1 = ay.i1 * a.w;
    int y[V], bi[V];
    if (sums) {
      const LT* lp = L + poff;
      dn_labels<V>(lp, n == V && (((uintptr_t)lp) & (sizeof(LT) == 8 ? 15u : 3u)) == 0, n, a.ignore, K, y);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = -1;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      bi[j] = 0;
      if (j >= n) continue;
      const UpAxis ax = up_axis(X0 + j, a.w, a.sx, a.align);
      float se = 1.f, zy = 0.f, py = 0.f;
      if constexpr (KT > 0) {
        float z[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) z[k] = up_tap<T>(x + k * a.sc, r0, r1, ax.i0, ax.i1, ay.l, ax.l);
#define DN_Z(k) z[k]
        DN_PIXEL(KT, DN_Z, y[j], true, bi[j], se, zy, py, rP, rI, rT);          // ignored pixels ARE branched around: in the prediction-only form every pixel is one
#undef DN_Z
      } else {
        // DELIBERATELY not dense_fwd_kernel's generic path: pixel-major over the taps (a class plane's four taps are not a 16-byte word), and an ignored
        // pixel is branched around, as above
        float best = up_tap<T>(x, r0, r1, ax.i0, ax.i1, ay.l, ax.l), m = best;
        int bb = 0;
        for (int k = 1; k < K; ++k) {
          const float z = up_tap<T>(x + k * a.sc, r0, r1, ax.i0, ax.i1, ay.l, ax.l);
          if (dn_better(z, best)) { best = z; bb = k; }
          m = fmaxf(m, z);
        }
        bi[j] = bb;
        if (y[j] >= 0) {
          float sum = 0.f;
          for (int k = 0; k < K; ++k) sum += expf(up_tap<T>(x + k * a.sc, r0, r1, ax.i0, ax.i1, ay.l, ax.l) - m);
          se = sum;
          const float inv = 1.f / sum;
          for (int k = 0; k < K; ++k) {
            const float dz = up_tap<T>(x + k * a.sc, r0, r1, ax.i0, ax.i1, ay.l, ax.l) - m;
            const float p = expf(dz) * inv;
            s.accP[k * NT + tid] += p;
            if (y[j] == k) { s.accI[k * NT + tid] += p; atomicAdd(&s.cntT[k], 1); zy = dz; py = p; }
          }
        }
      }
      dn_pixel_tail(a, a.t, K, s.conf, y[j], bi[j], se, zy, py, ce_sum, nll_sum, nvalid);
    }
    if (a.pred) dn_store_pred<V>(a.pred + poff, n == V && (((uintptr_t)(a.pred + poff)) & 3u) == 0, n, bi);          // rows start anywhere (W = 37): alignment per chunk
  }
  if (sums) dn_write_row<KT>(a.ws, a.conf, K, smem, s.red, s.cntT, s.conf, rP, rI, rT, ce_sum, nll_sum, nvalid);
}

// ---- sliding-window inference: stitch, resize and argmax in one pass -----------------------------------------------------------------------------------
// window logits [G, B, K, h, w] (G = gy gx windows of wh x ww image pixels, origins ys x xs, mmseg's order) -> per image pixel the MEAN over the covering windows
// of each window's bilinearly interpolated logits (mmseg's slide_inference: preds += pad(resize(logits)); preds / count_mat), evaluated per output pixel in fp32;
// from there it is dense_up_fwd_kernel's pixel.  The full-resolution map, the count map and the padded temporaries exist only if the caller asks for `mean`.
constexpr int SL_KREG = 8;          // K <= SL_KREG: the pixel's class means in registers (Potsdam / Vaihingen: 6, LoveDA: 7)
struct SlideArgs : DenseHead {
  int h, w, wh, ww, H, W, cpr, align, gy, gx;          // logits and window size, image size, chunks per image row
  int stash;          // generic path: the pixel's K means are kept in LDS ([K][threads] floats behind the forward layout) and not interpolated again per sweep
  float sy, sx;          // up_scale(h, wh), up_scale(w, ww)
  int64_t sg;          // window stride
  float* mean;          // nullable: fp32 [B, K, H, W]
  DenseTerms t;
  int ys[LMV_DENSE_SLIDE_MAX_GRID], xs[LMV_DENSE_SLIDE_MAX_GRID];
};

// THE stitching rule: f(window, r0, r1, c0, c1, ly, lx) for every window that covers image pixel (Y, X), in ascending (iy, ix) order -- mmseg's loop order, the
// order of its `preds +=`; returns their number (mmseg's count_mat).  The origins ascend: the first one behind the pixel ends the scan of an axis.
template <typename F> __device__ __forceinline__ int sl_windows(const SlideArgs& a, int Y, int X, F&& f) {
  int n = 0;
  for (int iy = 0; iy < a.gy; ++iy) {
    const int oy = Y - a.ys[iy];
    if (oy < 0) break;
    if (oy >= a.wh) continue;
    const UpAxis ay = up_axis(oy, a.h, a.sy, a.align);
    for (int ix = 0; ix < a.gx; ++ix) {
      const int ox = X - a.xs[ix];
      if (ox < 0) break;
      if (ox >= a.ww) continue;
      const UpAxis ax = up_axis(ox, a.w, a.sx, a.align);
      f(iy * a.gx + ix, ay.i0 * a.w, ay.i1 * a.w, ax.i0, ax.i1, ay.l, ax.l);
      ++n;
    }
  }
  return n;
}
// one class at one image pixel: the sum in window order, then THE division (a quotient can merge two sums into a tie that the first-index rule resolves)
template <typename T> __device__ __forceinline__ float sl_mean(const SlideArgs& a, const T* xk, int Y, int X) {
  float s = 0.f;
  const int n = sl_windows(a, Y, X, [&](int g, int r0, int r1, int c0, int c1, float ly, float lx) { s += up_tap<T>(xk + g * a.sg, r0, r1, c0, c1, ly, lx); });
  return s / (float)n;
}

// chunks, labels, LDS layout, pixel, row and summation discipline of dense_up_fwd_kernel; the covering set may change inside a chunk: it is evaluated per pixel.
// labels == NULL: prediction only (argmax map and / or the mean logits, no sums, no row).
template <typename T, typename LT, int KT> __global__ __launch_bounds__(256) void dense_slide_fwd_kernel(const SlideArgs a) {
  constexpr int V = UP_V;
  constexpr int KR = KT > 0 ? KT : 1;
  extern __shared__ float smem[];
  const int K = KT > 0 ? KT : a.K;
  const int NT = blockDim.x, tid = threadIdx.x;
  const bool sums = a.labels != nullptr;
  const DnLds s = dn_lds<KT>(smem, K, sums, a.conf != nullptr);
  float* st = (sums ? reinterpret_cast<float*>(s.conf + (a.conf ? K * K : 0)) : smem) + tid;          // the stash: st[k NT]
  float rP[KR], rI[KR];
  int rT[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) { rP[k] = 0.f; rI[k] = 0.f; rT[k] = 0; }
  float ce_sum = 0.f, nll_sum = 0.f;
  int nvalid = 0;
  const T* X = reinterpret_cast<const T*>(a.logits);
  const LT* L = reinterpret_cast<const LT*>(a.labels);
  const int64_t HW = (int64_t)a.H * a.W;

  for (int64_t ch = (int64_t)blockIdx.x * NT + tid; ch < a.nchunks; ch += (int64_t)gridDim.x * NT) {
    const int64_t orow = ch / a.cpr;          // b H + Y
    const int X0 = (int)(ch - orow * a.cpr) * V;
    const int b = (int)(orow / a.H), Y = (int)(orow - (int64_t)b * a.H);
    const int n = min(V, a.W - X0);
    const int64_t poff = orow * a.W + X0;
    const T* x = X + (int64_t)b * a.sb;
    int y[V], bi[V];
    if (sums) {
      const LT* lp = L + poff;
      dn_labels<V>(lp, n == V && (((uintptr_t)lp) & (sizeof(LT) == 8 ? 15u : 3u)) == 0, n, a.ignore, K, y);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = -1;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      bi[j] = 0;
      if (j >= n) continue;
      const int Xp = X0 + j;
      float* ml = a.mean ? a.mean + ((int64_t)b * K * HW + (int64_t)Y * a.W + Xp) : nullptr;          // class 0 of this pixel; one writer per element
      float se = 1.f, zy = 0.f, py = 0.f;
      if constexpr (KT > 0) {
        float z[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) z[k] = 0.f;
        const int cnt = sl_windows(a, Y, Xp, [&](int g, int r0, int r1, int c0, int c1, float ly, float lx) {
          const T* xw = x + g * a.sg;
#pragma unroll
          for (int k = 0; k < KT; ++k) z[k] += up_tap<T>(xw + k * a.sc, r0, r1, c0, c1, ly, lx);
        });
        const float fc = (float)cnt;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          z[k] = z[k] / fc;          // sl_mean's sum and division, all classes in one scan of the windows
          if (ml) ml[k * HW] = z[k];
        }
#define DN_Z(k) z[k]
        DN_PIXEL(KT, DN_Z, y[j], true, bi[j], se, zy, py, rP, rI, rT);          // ignored pixels ARE branched around, as in dense_up_fwd_kernel
#undef DN_Z
      } else {
        // dense_up_fwd_kernel's generic pixel over zk(k).  With the stash the windows are scanned once and each class interpolated once per window (sl_mean's sum
        // and division, through LDS); without it (the host's choice: K = 64 with sums and a confusion matrix leaves no room) every sweep interpolates again.
        if (a.stash) {
          for (int k = 0; k < K; ++k) st[k * NT] = 0.f;
          const int cnt = sl_windows(a, Y, Xp, [&](int g, int r0, int r1, int c0, int c1, float ly, float lx) {
            const T* xw = x + g * a.sg;
            for (int k = 0; k < K; ++k) st[k * NT] += up_tap<T>(xw + k * a.sc, r0, r1, c0, c1, ly, lx);
          });
          const float fc = (float)cnt;
          for (int k = 0; k < K; ++k) st[k * NT] = st[k * NT] / fc;
        }
        auto zk = [&](int k) { return a.stash ? st[k * NT] : sl_mean<T>(a, x + k * a.sc, Y, Xp); };
        float best = zk(0), m = best;
        int bb = 0;
        if (ml) ml[0] = best;
        for (int k = 1; k < K; ++k) {
          const float z = zk(k);
          if (ml) ml[k * HW] = z;
          if (dn_better(z, best)) { best = z; bb = k; }
          m = fmaxf(m, z);
        }
        bi[j] = bb;
        if (y[j] >= 0) {
          float sum = 0.f;
          for (int k = 0; k < K; ++k) sum += expf(zk(k) - m);
          se = sum;
          const float inv = 1.f / sum;
          for (int k = 0; k < K; ++k) {
            const float dz = zk(k) - m;
            const float p = expf(dz) * inv;
            s.accP[k * NT + tid] += p;
            if (y[j] == k) { s.accI[k * NT + tid] += p; atomicAdd(&s.cntT[k], 1); zy = dz; py = p; }
          }
        }
      }
      dn_pixel_tail(a, a.t, K, s.conf, y[j], bi[j], se, zy, py, ce_sum, nll_sum, nvalid);
    }
    if (a.pred) dn_store_pred<V>(a.pred + poff, n == V && (((uintptr_t)(a.pred + poff)) & 3u) == 0, n, bi);
  }
  if (sums) dn_write_row<KT>(a.ws, a.conf, K, smem, s.red, s.cntT, s.conf, rP, rI, rT, ce_sum, nll_sum, nvalid);
}

// ---- backward: ONE launch, every element of dlogits [B, K, h, w] written once, no atomics ----
// A workgroup owns a tile of TH x TW input pixels of one image.  The output pixels that touch the tile (its footprint: a rectangle, found with up_first / up_end)
// are taken in blocks of at most FBH x FBW.  Per block: (1) one sweep leaves every output pixel's max, 1 / sum, sum_j p_j g_j, the CE factor and the label in
// LDS; (2) per class, the block's dz_high plane goes to LDS (two buffers: one barrier per class) and G threads per input pixel gather
// wy wx dz_high (weights from two small per-block tables) over that pixel's rows of the block in a fixed order, a butterfly over the G threads, and the group's first thread adds the block's sum to the
// pixel's accumulator in LDS.  The softmax is evaluated once per output pixel and block; the fixed orders make two calls agree bit for bit.
// LDS (dynamic, floats): max | 1/sum | sg | cf | label [FB] each | plane [2][FB] | acc [K][TH TW] | axis tables y: i0, i1, l [FBH], x: i0, i1, l [FBW] | weights [TH][FBH], [TW][FBW] | ranges [32] | STAGE: logits [K][TH + 2][TW + 2]
template <typename T, typename LT, bool STAGE> __global__ __launch_bounds__(256) void dense_up_bwd_kernel(const UpArgs a) {
  extern __shared__ float smem[];
  const int K = a.K, tid = threadIdx.x, NT = 256;
  const int FB = a.FBH * a.FBW, TP = a.TH * a.TW;
  float* sM = smem;
  float* sInv = sM + FB;
  float* sSg = sInv + FB;
  float* sCf = sSg + FB;
  int* sY = reinterpret_cast<int*>(sCf + FB);
  float* plane = reinterpret_cast<float*>(sY + FB);
  float* acc = plane + 2 * FB;
  int* yI0 = reinterpret_cast<int*>(acc + K * TP);
  int* yI1 = yI0 + a.FBH;
  float* yL = reinterpret_cast<float*>(yI1 + a.FBH);
  int* xI0 = reinterpret_cast<int*>(yL + a.FBH);
  int* xI1 = xI0 + a.FBW;
  float* xL = reinterpret_cast<float*>(xI1 + a.FBW);
  float* wyT = xL + a.FBW;          // [TH][FBH]: the weight of tile row t in block row i
  float* wxT = wyT + a.TH * a.FBH;          // [TW][FBW]
  int* rng = reinterpret_cast<int*>(wxT + a.TW * a.FBW);          // rLo [8] | rHi [8] | cLo [8] | cHi [8]
  float* stage = reinterpret_cast<float*>(rng + 32);          // STAGE: [K][sh][sw], the tile's logits and a halo of one input pixel, as floats

  const int tx_i = blockIdx.x % a.tiles_x, ty_i = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int ty0 = ty_i * a.TH, tx0 = tx_i * a.TW;
  const int th = min(a.TH, a.h - ty0), tw = min(a.TW, a.w - tx0);
  const int Ylo = up_first(ty0, a.h, a.H, a.sy, a.align), Yhi = up_end(ty0 + th - 1, a.h, a.H, a.sy, a.align);
  const int Xlo = up_first(tx0, a.w, a.W, a.sx, a.align), Xhi = up_end(tx0 + tw - 1, a.w, a.W, a.sx, a.align);

  const T* x = reinterpret_cast<const T*>(a.logits) + (int64_t)b * a.sb;
  // every output pixel of the footprint has its taps in input rows [ty0 - 1, ty0 + th] and columns [tx0 - 1, tx0 + tw] (i1 <= i0 + 1), clamped to the image.
  // STAGE (the host's choice: it fits into LDS): these logits are read from global memory once; otherwise every tap is a cached global load.  The values are the same.
  const int y0s = STAGE ? max(ty0 - 1, 0) : 0, x0s = STAGE ? max(tx0 - 1, 0) : 0;
  const int sh = min(ty0 + th, a.h - 1) - y0s + 1, sw = min(tx0 + tw, a.w - 1) - x0s + 1;
  using ZT = typename std::conditional<STAGE, float, T>::type;
  const ZT* zb = STAGE ? reinterpret_cast<const ZT*>(stage) : reinterpret_cast<const ZT*>(x);
  const int zpitch = STAGE ? sw : a.w;
  const int64_t zk = STAGE ? (int64_t)sh * sw : a.sc;
  if (STAGE) {
    for (int e = tid; e < K * sh * sw; e += NT) {
      const int k = e / (sh * sw), r = e - k * (sh * sw);
      const int yy = r / sw, xx = r - yy * sw;
      stage[e] = DT<T>::ld(x + k * a.sc + (int64_t)(y0s + yy) * a.w + (x0s + xx));
    }
  }
  const LT* L = reinterpret_cast<const LT*>(a.labels) + (int64_t)b * a.H * a.W;
  const float gout = a.gout ? *a.gout : 1.f;
  const float invD = a.stats[5];
  const float* U = a.stats + LMV_DENSE_STATS_HEAD;
  const float* Vt = U + K;
  // the gather's thread -> (input pixel, part)
  const int gp = tid / a.G, part = tid - gp * a.G;
  const int gy = gp / a.TW, gx = gp - gy * a.TW;
  const bool gather = gp < TP && gy < th && gx < tw;

  for (int i = tid; i < K * TP; i += NT) acc[i] = 0.f;
  // the footprint in equal blocks of at most FBH x FBW (no sliver at the end)
  const int nby = (Yhi - Ylo + a.FBH - 1) / a.FBH, nbx = (Xhi - Xlo + a.FBW - 1) / a.FBW;
  const int sby = (Yhi - Ylo + nby - 1) / nby, sbx = (Xhi - Xlo + nbx - 1) / nbx;
  for (int Yb = Ylo; Yb < Yhi; Yb += sby) {
    const int bh = min(sby, Yhi - Yb);
    for (int Xb = Xlo; Xb < Xhi; Xb += sbx) {
      const int bw = min(sbx, Xhi - Xb);
      __syncthreads();          // the previous block's gather is over: tables, scalars and planes may be overwritten
      for (int i = tid; i < bh + bw; i += NT) {
        if (i < bh) {
          const UpAxis ax = up_axis(Yb + i, a.h, a.sy, a.align);
          yI0[i] = ax.i0; yI1[i] = ax.i1; yL[i] = ax.l;
          for (int t = 0; t < a.TH; ++t) wyT[t * a.FBH + i] = up_weight(ax.i0, ax.i1, ax.l, ty0 + t);
        } else {
          const int j = i - bh;
          const UpAxis ax = up_axis(Xb + j, a.w, a.sx, a.align);
          xI0[j] = ax.i0; xI1[j] = ax.i1; xL[j] = ax.l;
          for (int t = 0; t < a.TW; ++t) wxT[t * a.FBW + j] = up_weight(ax.i0, ax.i1, ax.l, tx0 + t);
        }
      }
      __syncthreads();
      if (tid < 16) {          // the rows (tid < 8) / columns of the block that touch tile row / column tid & 7: contiguous, possibly empty
        const int t = tid & 7, isx = tid >> 3;
        const int idx = (isx ? tx0 : ty0) + t, cnt = isx ? bw : bh;
        const int* I0 = isx ? xI0 : yI0;
        const int* I1 = isx ? xI1 : yI1;
        int lo = cnt, hi = 0;
        for (int i = 0; i < cnt; ++i)
          if (I0[i] == idx || I1[i] == idx) { lo = min(lo, i); hi = i + 1; }
        if (lo > hi) lo = hi;
        rng[isx * 16 + t] = lo; rng[isx * 16 + 8 + t] = hi;
      }
      // (1) the scalars of every output pixel of the block
      for (int f = tid; f < bh * bw; f += NT) {
        const int Yr = f / bw, Xr = f - Yr * bw;
        int yv;
        dn_labels<1>(L + (int64_t)(Yb + Yr) * a.W + (Xb + Xr), false, 1, a.ignore, K, &yv);
        sY[f] = yv;
        if (yv < 0) continue;
        const int r0 = (yI0[Yr] - y0s) * zpitch, r1 = (yI1[Yr] - y0s) * zpitch, c0 = xI0[Xr] - x0s, c1 = xI1[Xr] - x0s;
        const float ly = yL[Yr], lx = xL[Xr];
        float m = up_tap<ZT>(zb, r0, r1, c0, c1, ly, lx);
        for (int k = 1; k < K; ++k) m = fmaxf(m, up_tap<ZT>(zb + k * zk, r0, r1, c0, c1, ly, lx));
        float s = 0.f, ey = 0.f, sgu = 0.f;
        for (int k = 0; k < K; ++k) {
          const float e = expf(up_tap<ZT>(zb + k * zk, r0, r1, c0, c1, ly, lx) - m);
          const bool hit = yv == k;
          s += e;
          if (hit) ey = e;
          if (a.t.shape_terms) sgu += e * dn_shape(hit, U[k], Vt[k]);
        }
        const float inv = 1.f / s;
        // DELIBERATELY not dense_bwd_kernel's order: sg = (sum_k e_k (v_k + [hit] u_k)) inv and p_y = e_y inv, one multiply per pixel instead of one per class
        sM[f] = m; sInv[f] = inv; sSg[f] = sgu * inv;
        sCf[f] = dn_cf(a, a.t, invD, yv, ey * inv);
      }
      __syncthreads();
      const int rl = gather ? rng[gy] : 0, rh = gather ? rng[8 + gy] : 0, cl = gather ? rng[16 + gx] : 0, chh = gather ? rng[24 + gx] : 0;
      const float* wyG = wyT + gy * a.FBH;
      const float* wxG = wxT + gx * a.FBW;
      // (2) per class: plane, barrier, gather
      for (int k = 0; k < K; ++k) {
        float* pl = plane + (k & 1) * FB;
        const float uk = U[k], vk = Vt[k];          // once per class, in front of the pixel loop: this kernel has no scalar register to spare for reads inside it
        for (int f = tid; f < bh * bw; f += NT) {
          const int yv = sY[f];
          float g = 0.f;
          if (yv >= 0) {
            const int Yr = f / bw, Xr = f - Yr * bw;
            const float z = up_tap<ZT>(zb + k * zk, (yI0[Yr] - y0s) * zpitch, (yI1[Yr] - y0s) * zpitch, xI0[Xr] - x0s, xI1[Xr] - x0s, yL[Yr], xL[Xr]);
            g = dn_grad(a.t, expf(z - sM[f]) * sInv[f], yv == k, sCf[f], &uk, &vk, 0, sSg[f], gout);
          }
          pl[f] = g;
        }
        __syncthreads();
        float s = 0.f;
        for (int Yr = rl + part; Yr < rh; Yr += a.G) {          // the group's threads take the pixel's block rows in turn, each row left to right
          const float* pr = pl + Yr * bw;
          float sr = 0.f;
          for (int Xr = cl; Xr < chh; ++Xr) sr += wxG[Xr] * pr[Xr];
          s += wyG[Yr] * sr;
        }
        for (int o = a.G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (gather && part == 0) acc[k * TP + gp] += s;
      }
    }
  }
  __syncthreads();
  T* DL = reinterpret_cast<T*>(a.dlogits);
  for (int e = tid; e < K * TP; e += NT) {
    const int k = e / TP, p = e - k * TP;
    const int py = p / a.TW, px = p - py * a.TW;
    if (py < th && px < tw) DT<T>::st(DL + (((int64_t)b * K + k) * a.h + (ty0 + py)) * a.w + (tx0 + px), acc[e]);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------
static int dn_rows(int B, int K, int64_t HW, int V, int cap) {
  const int64_t nchunks = (int64_t)B * dn_cdiv(HW, V);
  return (int)std::min<int64_t>(dn_cdiv(nchunks, dn_threads(K)), cap);
}

static int dn_validate(const char* fn, const void* logits, int dtype, int64_t sb, int64_t sc, int B, int K, int64_t HW, const void* labels, int label_dtype,
                       const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps, int avg_mode) {
  if (!logits || !labels) LMV_FAIL(LMV_ERR_SHAPE, "%s: null logits / labels", fn);
  if (K < 2 || K > LMV_DENSE_MAX_CLASSES) LMV_FAIL(LMV_ERR_SHAPE, "%s: K = %d classes outside 2 .. %d", fn, K, LMV_DENSE_MAX_CLASSES);
  if (B < 1 || HW < 1 || (int64_t)B * HW >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape B = %d, H W = %lld (B >= 1, H W >= 1, B H W < 2^31)", fn, B, (long long)HW);
  if (dtype != LMV_F32 && dtype != LMV_BF16) LMV_FAIL(LMV_ERR_SHAPE, "%s: unsupported logits dtype code %d (fp32 / bf16)", fn, dtype);
  if (label_dtype != LMV_DENSE_LABEL_I64 && label_dtype != LMV_DENSE_LABEL_U8) LMV_FAIL(LMV_ERR_SHAPE, "%s: unsupported label dtype code %d (int64 / uint8)", fn, label_dtype);
  if (sc < HW) LMV_FAIL(LMV_ERR_SHAPE, "%s: class stride %lld < H W = %lld", fn, (long long)sc, (long long)HW);
  if (sb < (int64_t)(K - 1) * sc + HW) LMV_FAIL(LMV_ERR_SHAPE, "%s: batch stride %lld < the %d class planes it skips", fn, (long long)sb, K);
  if (!(w_ce >= 0.f) || !(w_dice >= 0.f) || !(w_jac >= 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: negative loss weight (%g, %g, %g)", fn, w_ce, w_dice, w_jac);
  if (!(gamma >= 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: gamma = %g < 0", fn, gamma);
  if (!(eps > 0.f)) LMV_FAIL(LMV_ERR_SHAPE, "%s: eps = %g <= 0", fn, eps);
  if (avg_mode != LMV_DENSE_AVG_VALID && avg_mode != LMV_DENSE_AVG_ALL && avg_mode != LMV_DENSE_AVG_WEIGHT) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown avg_mode %d", fn, avg_mode);
  if ((((uintptr_t)logits) & (dtype == LMV_F32 ? 3u : 1u)) || (label_dtype == LMV_DENSE_LABEL_I64 && (((uintptr_t)labels) & 7u)) || (((uintptr_t)alpha) & 3u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  return LMV_OK;
}

// the common head of both argument structs
static void dn_head(DenseHead& a, DenseTerms& t, const void* logits, int64_t sb, int64_t sc, int B, int K, const void* labels, int64_t ignore, const float* alpha, float gamma,
                    float w_ce, float w_dice, float w_jac) {
  a.logits = logits; a.labels = labels; a.alpha = alpha;
  a.sb = sb; a.sc = sc; a.ignore = ignore;
  a.B = B; a.K = K;
  t.gamma = gamma; t.w_ce = w_ce; t.shape_terms = (w_dice != 0.f || w_jac != 0.f) ? 1 : 0;
}

static DenseArgs dn_args(const void* logits, int dtype, int64_t sb, int64_t sc, int B, int K, int64_t HW, const void* labels, int label_dtype, int64_t ignore,
                         const float* alpha, float gamma, float w_ce, float w_dice, float w_jac) {
  const int V = dtype == LMV_F32 ? 4 : 8;
  DenseArgs a = {};
  dn_head(a, a.t, logits, sb, sc, B, K, labels, ignore, alpha, gamma, w_ce, w_dice, w_jac);
  a.HW = (int)HW; a.cpi = (int)dn_cdiv(HW, V);
  a.nchunks = (int64_t)B * a.cpi;
  a.xvec = lmv_aligned16(logits) && sb % V == 0 && sc % V == 0;
  a.lvec = lmv_aligned16(labels) && HW % V == 0;
  return a;
}

// ---- the checks and the second launch that the four entry points share; fn: the entry point's name, the head of every message ----
static int dn_check_fwd(const char* fn, const char* sizer, const void* workspace, size_t workspace_bytes, int rows, int K, const float* stats, const int64_t* conf, const double* meter) {
  if (!workspace || !stats) LMV_FAIL(LMV_ERR_SHAPE, "%s: null workspace / stats", fn);
  if ((((uintptr_t)workspace) & 3u) || (((uintptr_t)stats) & 3u) || (((uintptr_t)conf) & 7u) || (((uintptr_t)meter) & 7u)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  const size_t need = (size_t)rows * (size_t)(3 * K + 3) * sizeof(float);
  if (workspace_bytes < need) LMV_FAIL(LMV_ERR_SHAPE, "%s: workspace of %zu bytes, %zu needed (%s)", fn, workspace_bytes, need, sizer);
  return LMV_OK;
}

static int dn_check_bwd(const char* fn, int dtype, const float* stats, const float* gout, const void* dlogits) {
  if (!stats || !dlogits) LMV_FAIL(LMV_ERR_SHAPE, "%s: null stats / dlogits", fn);
  if ((((uintptr_t)stats) & 3u) || (((uintptr_t)gout) & 3u) || (((uintptr_t)dlogits) & (dtype == LMV_F32 ? 3u : 1u))) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  return LMV_OK;
}

static int dn_finalize(const char* fn, const float* ws, int rows, int K, double npix, const float* alpha, float w_ce, float w_dice, float w_jac, float eps,
                       int avg_mode, float* stats, double* meter, hipStream_t st) {
  DenseFinArgs f;
  f.ws = ws; f.alpha = alpha; f.stats = stats; f.meter = meter; f.rows = rows; f.K = K; f.avg_mode = avg_mode;
  f.npix = npix; f.w_ce = w_ce; f.w_dice = w_dice; f.w_jac = w_jac; f.eps = eps;
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(1), dim3(256), 0, st, f);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s (finalize): %s", fn, hipGetErrorString(e));
  return LMV_OK;
}

// THE type switch of every launch here: f(T(), LT()) with the logits' and the labels' element types as (value-less) tags
template <typename F> static void dn_for_types(int dtype, int label_dtype, F&& f) {
  if (dtype == LMV_F32) {
    if (label_dtype == LMV_DENSE_LABEL_I64) f(float(), int64_t()); else f(float(), uint8_t());
  } else {
    if (label_dtype == LMV_DENSE_LABEL_I64) f(bf16_t(), int64_t()); else f(bf16_t(), uint8_t());
  }
}
#define DN_FOR_K(KERNEL, T, LT, ...)                                                              \
  switch (a.K <= DN_KREG ? a.K : 0) {                                                             \
    case 2: hipLaunchKernelGGL((KERNEL<T, LT, 2>), __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL((KERNEL<T, LT, 3>), __VA_ARGS__); break;                           \
    case 4: hipLaunchKernelGGL((KERNEL<T, LT, 4>), __VA_ARGS__); break;                           \
    case 5: hipLaunchKernelGGL((KERNEL<T, LT, 5>), __VA_ARGS__); break;                           \
    default: hipLaunchKernelGGL((KERNEL<T, LT, 0>), __VA_ARGS__); break;                          \
  }
#define DN_DISPATCH(KERNEL, ...) \
  dn_for_types(dtype, label_dtype, [&](auto t, auto l) { DN_FOR_K(KERNEL, decltype(t), decltype(l), __VA_ARGS__) })
}  // namespace

extern "C" size_t lmv_dense_loss_workspace_bytes(int B, int K, int64_t HW) {
  if (B < 1 || HW < 1 || K < 2 || K > LMV_DENSE_MAX_CLASSES || (int64_t)B * HW >= (1ll << 31)) return 0;
  return (size_t)dn_rows(B, K, HW, 4, DN_MAX_WG) * (size_t)(3 * K + 3) * sizeof(float);          // (bf16: 8 pixels per chunk, fewer rows)
}

extern "C" int lmv_dense_loss_fwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels,
                                  int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps,
                                  int avg_mode, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred, int64_t* conf, double* meter, void* stream) {
  const char* fn = "dense_loss_fwd";
  if (int rc = dn_validate(fn, logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, alpha, gamma, w_ce, w_dice, w_jac, eps, avg_mode)) return rc;
  const int V = dtype == LMV_F32 ? 4 : 8;
  const int rows = dn_rows(B, K, HW, V, DN_MAX_WG), NT = dn_threads(K);
  if (int rc = dn_check_fwd(fn, "lmv_dense_loss_workspace_bytes", workspace, workspace_bytes, rows, K, stats, conf, meter)) return rc;
  DenseArgs a = dn_args(logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.ws = reinterpret_cast<float*>(workspace); a.pred = pred; a.conf = reinterpret_cast<unsigned long long*>(conf);
  a.pvec = pred && (((uintptr_t)pred) & 7u) == 0 && HW % V == 0;
  hipStream_t st = (hipStream_t)stream;
  DN_DISPATCH(dense_fwd_kernel, dim3(rows), dim3(NT), dn_lds_bytes(K, NT, conf != nullptr), st, a);
  LMV_CHECK_LAUNCH(fn);
  return dn_finalize(fn, a.ws, rows, K, (double)B * (double)HW, alpha, w_ce, w_dice, w_jac, eps, avg_mode, stats, meter, st);
}

extern "C" int lmv_dense_loss_bwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels,
                                  int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps,
                                  int avg_mode, const float* stats, const float* gout, void* dlogits, void* stream) {
  const char* fn = "dense_loss_bwd";
  if (int rc = dn_validate(fn, logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, alpha, gamma, w_ce, w_dice, w_jac, eps, avg_mode)) return rc;
  if (int rc = dn_check_bwd(fn, dtype, stats, gout, dlogits)) return rc;
  const int V = dtype == LMV_F32 ? 4 : 8;
  DenseArgs a = dn_args(logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.stats = stats; a.gout = gout; a.dlogits = dlogits;
  a.dvec = lmv_aligned16(dlogits) && HW % V == 0;
  const int NT = 256, rows = (int)std::min<int64_t>(dn_cdiv(a.nchunks, NT), DN_MAX_WG_BWD);
  DN_DISPATCH(dense_bwd_kernel, dim3(rows), dim3(NT), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

// ---- the upsampling entry points ----
namespace {
static int up_rows(int B, int K, int H, int W) {
  const int64_t nchunks = (int64_t)B * H * dn_cdiv(W, UP_V);
  return (int)std::min<int64_t>(dn_cdiv(nchunks, dn_threads(K)), DN_MAX_WG);
}

static int up_validate(const char* fn, const void* logits, int dtype, int64_t sb, int64_t sc, int B, int K, int h, int w, int H, int W, int align_corners,
                       const void* labels, bool need_labels, int label_dtype, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps,
                       int avg_mode) {
  if (h < 1 || w < 1 || H < h || W < w)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: bad sizes %d x %d -> %d x %d (h >= 1, w >= 1, H >= h, W >= w: upsampling only)", fn, h, w, H, W);
  if (B >= 1 && (int64_t)B * H * W >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad shape B = %d, H W = %lld (B H W < 2^31)", fn, B, (long long)H * W);
  if (align_corners != 0 && align_corners != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: align_corners = %d is neither 0 nor 1", fn, align_corners);
  if (!labels && !need_labels) { labels = logits; label_dtype = LMV_DENSE_LABEL_U8; }          // prediction only: no label map to check
  return dn_validate(fn, logits, dtype, sb, sc, B, K, (int64_t)h * w, labels, label_dtype,
                     alpha, gamma, w_ce, w_dice, w_jac, eps, avg_mode);
}

static float up_scale(int in, int out, int align) { return align ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out; }

// one axis of the backward's tiling: the largest tile of 8, 4, 2, 1 input indices whose footprint of about (T + 1) out / in output indices is at most two blocks
// of UP_FB (the softmax of the footprint's margin is evaluated by the neighbouring tiles too: (T + 1)^2 / T^2 of the work, so a larger tile in more blocks wins)
static void up_tile(int in, int out, int* T, int* FBd) {
  const int r = (out + in - 1) / in;
  int t = 8;
  while (t > 1 && ((t + 1) * r > 2 * UP_FB || t >= 2 * in)) t >>= 1;
  *T = t;
  *FBd = std::min(std::min(UP_FB, (t + 1) * r + 2), out);
}

static UpArgs up_args(const void* logits, int64_t sb, int64_t sc, int B, int K, int h, int w, int H, int W, int align, const void* labels, int64_t ignore,
                      const float* alpha, float gamma, float w_ce, float w_dice, float w_jac) {
  UpArgs a = {};
  dn_head(a, a.t, logits, sb, sc, B, K, labels, ignore, alpha, gamma, w_ce, w_dice, w_jac);
  a.h = h; a.w = w; a.H = H; a.W = W; a.align = align;
  a.cpr = (int)dn_cdiv(W, UP_V); a.nchunks = (int64_t)B * H * a.cpr;
  a.sy = up_scale(h, H, align); a.sx = up_scale(w, W, align);
  return a;
}
}  // namespace

extern "C" size_t lmv_dense_up_loss_workspace_bytes(int B, int K, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || K < 2 || K > LMV_DENSE_MAX_CLASSES || (int64_t)B * H * W >= (1ll << 31)) return 0;
  return (size_t)up_rows(B, K, H, W) * (size_t)(3 * K + 3) * sizeof(float);
}

extern "C" int lmv_dense_up_loss_fwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w, int H, int W,
                                     int align_corners, const void* labels, int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce,
                                     float w_dice, float w_jac, float eps, int avg_mode, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred,
                                     int64_t* conf, double* meter, void* stream) {
  const char* fn = "dense_up_loss_fwd";
  if (!labels && !pred && logits) LMV_FAIL(LMV_ERR_SHAPE, "%s: null labels and null pred: nothing to compute", fn);
  if (int rc = up_validate(fn, logits, dtype, batch_stride, class_stride, B, K, h, w, H, W, align_corners, labels, pred == nullptr, label_dtype, alpha, gamma, w_ce,
                           w_dice, w_jac, eps, avg_mode)) return rc;
  const int rows = up_rows(B, K, H, W), NT = dn_threads(K);
  if (labels)
    if (int rc = dn_check_fwd(fn, "lmv_dense_up_loss_workspace_bytes", workspace, workspace_bytes, rows, K, stats, conf, meter)) return rc;
  UpArgs a = up_args(logits, batch_stride, class_stride, B, K, h, w, H, W, align_corners, labels, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.ws = reinterpret_cast<float*>(workspace); a.pred = pred; a.conf = labels ? reinterpret_cast<unsigned long long*>(conf) : nullptr;
  if (!labels) label_dtype = LMV_DENSE_LABEL_U8;
  hipStream_t st = (hipStream_t)stream;
  DN_DISPATCH(dense_up_fwd_kernel, dim3(rows), dim3(NT), dn_lds_bytes(K, NT, a.conf != nullptr), st, a);
  LMV_CHECK_LAUNCH(fn);
  if (!labels) return LMV_OK;
  return dn_finalize(fn, a.ws, rows, K, (double)B * (double)H * (double)W, alpha, w_ce, w_dice, w_jac, eps, avg_mode, stats, meter, st);
}

extern "C" int lmv_dense_up_loss_bwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w, int H, int W,
                                     int align_corners, const void* labels, int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce,
                                     float w_dice, float w_jac, float eps, int avg_mode, const float* stats, const float* gout, void* dlogits, void* stream) {
  const char* fn = "dense_up_loss_bwd";
  if (int rc = up_validate(fn, logits, dtype, batch_stride, class_stride, B, K, h, w, H, W, align_corners, labels, true, label_dtype, alpha, gamma, w_ce, w_dice,
                           w_jac, eps, avg_mode)) return rc;
  if (int rc = dn_check_bwd(fn, dtype, stats, gout, dlogits)) return rc;
  UpArgs a = up_args(logits, batch_stride, class_stride, B, K, h, w, H, W, align_corners, labels, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.stats = stats; a.gout = gout; a.dlogits = dlogits;
  up_tile(h, H, &a.TH, &a.FBH);
  up_tile(w, W, &a.TW, &a.FBW);
  a.tiles_y = (int)dn_cdiv(h, a.TH); a.tiles_x = (int)dn_cdiv(w, a.TW);
  const int TP = a.TH * a.TW;
  a.G = std::min(64, 256 / TP);
  const size_t lds = ((size_t)7 * a.FBH * a.FBW + (size_t)K * TP + 3 * (size_t)(a.FBH + a.FBW) + (size_t)a.TH * a.FBH + (size_t)a.TW * a.FBW + 32) * sizeof(float);
  const size_t lds_stage = lds + (size_t)K * (a.TH + 2) * (a.TW + 2) * sizeof(float);          // the logits tile too, where the default 64 KB of LDS hold it
  const dim3 grid((unsigned)((int64_t)B * a.tiles_y * a.tiles_x));
  const bool stage = lds_stage <= 65536;
  dn_for_types(dtype, label_dtype, [&](auto t, auto l) {
    if (stage) hipLaunchKernelGGL((dense_up_bwd_kernel<decltype(t), decltype(l), true>), grid, dim3(256), lds_stage, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((dense_up_bwd_kernel<decltype(t), decltype(l), false>), grid, dim3(256), lds, (hipStream_t)stream, a);
  });
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

// ---- the sliding-window entry points ----
extern "C" size_t lmv_dense_slide_workspace_bytes(int B, int K, int H, int W) { return lmv_dense_up_loss_workspace_bytes(B, K, H, W); }          // the same chunks, the same rows

namespace {
static int sl_check_axis(const char* fn, const char* axis, const int* o, int g, int win, int img) {
  if (g < 1 || g > LMV_DENSE_SLIDE_MAX_GRID) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d windows along %s outside 1 .. %d", fn, g, axis, LMV_DENSE_SLIDE_MAX_GRID);
  if (!o) LMV_FAIL(LMV_ERR_SHAPE, "%s: null window origins along %s", fn, axis);
  for (int i = 1; i < g; ++i)
    if (o[i] <= o[i - 1]) LMV_FAIL(LMV_ERR_SHAPE, "%s: window origins along %s are not strictly increasing (%d after %d)", fn, axis, o[i], o[i - 1]);
  if (o[0] != 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: the first window along %s starts at %d, not at 0", fn, axis, o[0]);
  if ((int64_t)o[g - 1] + win != img) LMV_FAIL(LMV_ERR_SHAPE, "%s: the last window along %s ends at %lld, the image at %d", fn, axis, (long long)o[g - 1] + win, img);
  for (int i = 1; i < g; ++i)
    if (o[i] - o[i - 1] > win) LMV_FAIL(LMV_ERR_SHAPE, "%s: a gap along %s: windows of %d at %d and %d leave pixels uncovered", fn, axis, win, o[i - 1], o[i]);
  return LMV_OK;
}
#define SL_FOR_K(T, LT, ...)                                                                                  \
  switch (a.K <= SL_KREG ? a.K : 0) {                                                                         \
    case 2: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 2>), __VA_ARGS__); break;                       \
    case 3: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 3>), __VA_ARGS__); break;                       \
    case 4: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 4>), __VA_ARGS__); break;                       \
    case 5: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 5>), __VA_ARGS__); break;                       \
    case 6: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 6>), __VA_ARGS__); break;                       \
    case 7: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 7>), __VA_ARGS__); break;                       \
    case 8: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 8>), __VA_ARGS__); break;                       \
    default: hipLaunchKernelGGL((dense_slide_fwd_kernel<T, LT, 0>), __VA_ARGS__); break;                      \
  }
}  // namespace

extern "C" int lmv_dense_slide_fwd(const void* logits, int dtype, int64_t window_stride, int64_t batch_stride, int64_t class_stride, int B, int K, int h, int w,
                                   const int* ys, int gy, const int* xs, int gx, int wh, int ww, int H, int W, int align_corners, const void* labels,
                                   int label_dtype, int64_t ignore_index, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred,
                                   float* mean_logits, int64_t* conf, double* meter, void* stream) {
  const char* fn = "dense_slide_fwd";
  if (!labels && !pred && !mean_logits && logits) LMV_FAIL(LMV_ERR_SHAPE, "%s: null labels, null pred and null mean_logits: nothing to compute", fn);
  // per window it is the upsampling forward, h x w -> wh x ww (h > wh or w > ww: downsampling, refused there)
  if (int rc = up_validate(fn, logits, dtype, batch_stride, class_stride, B, K, h, w, wh, ww, align_corners, labels, !pred && !mean_logits, label_dtype, nullptr, 0.f,
                           1.f, 0.f, 0.f, 1e-7f, LMV_DENSE_AVG_VALID)) return rc;
  if (H < 1 || W < 1 || (int64_t)B * H * W >= (1ll << 31)) LMV_FAIL(LMV_ERR_SHAPE, "%s: bad image size %d x %d (H >= 1, W >= 1, B H W < 2^31)", fn, H, W);
  if (int rc = sl_check_axis(fn, "y", ys, gy, wh, H)) return rc;
  if (int rc = sl_check_axis(fn, "x", xs, gx, ww, W)) return rc;
  if (window_stride < (int64_t)(B - 1) * batch_stride + (int64_t)(K - 1) * class_stride + (int64_t)h * w)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: window stride %lld < the %d images it skips", fn, (long long)window_stride, B);
  if (((uintptr_t)mean_logits) & 3u) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  const int rows = up_rows(B, K, H, W), NT = dn_threads(K);
  if (labels)
    if (int rc = dn_check_fwd(fn, "lmv_dense_slide_workspace_bytes", workspace, workspace_bytes, rows, K, stats, conf, meter)) return rc;
  SlideArgs a = {};
  dn_head(a, a.t, logits, batch_stride, class_stride, B, K, labels, ignore_index, nullptr, 0.f, 1.f, 0.f, 0.f);          // an evaluation pass: plain cross-entropy
  a.h = h; a.w = w; a.wh = wh; a.ww = ww; a.H = H; a.W = W; a.align = align_corners; a.gy = gy; a.gx = gx; a.sg = window_stride;
  a.cpr = (int)dn_cdiv(W, UP_V); a.nchunks = (int64_t)B * H * a.cpr;
  a.sy = up_scale(h, wh, align_corners); a.sx = up_scale(w, ww, align_corners);
  std::copy(ys, ys + gy, a.ys); std::copy(xs, xs + gx, a.xs);
  a.ws = reinterpret_cast<float*>(workspace); a.pred = pred; a.mean = mean_logits; a.conf = labels ? reinterpret_cast<unsigned long long*>(conf) : nullptr;
  if (!labels) label_dtype = LMV_DENSE_LABEL_U8;
  size_t lds = labels ? dn_lds_bytes(K, NT, a.conf != nullptr, SL_KREG) : 0;
  const size_t stash = K > SL_KREG ? (size_t)K * NT * sizeof(float) : 0;
  a.stash = stash && lds + stash <= 65536;
  if (a.stash) lds += stash;
  hipStream_t st = (hipStream_t)stream;
  dn_for_types(dtype, label_dtype, [&](auto t, auto l) { SL_FOR_K(decltype(t), decltype(l), dim3(rows), dim3(NT), lds, st, a) });
  LMV_CHECK_LAUNCH(fn);
  if (!labels) return LMV_OK;
  return dn_finalize(fn, a.ws, rows, K, (double)B * (double)H * (double)W, nullptr, 1.f, 0.f, 0.f, 1e-7f, LMV_DENSE_AVG_VALID, stats, meter, st);
}
