// dense.hip -- the losses and metrics behind a dense-prediction head (the reference's change_detection/utils/metrics.py FocalLoss / dice_loss / jaccard_loss and
// utils/losses.py hybrid_loss, train.py:154-260, eval.py:39-66; the segmentation heads' per-pixel cross-entropy with an ignore index and the mIoU histogram):
//   lmv_dense_loss_fwd: (a) ONE pass over NCHW logits and a label map -> per workgroup one row of fp32 partial sums (P_k, I_k, T_k, the weighted and the plain
//                       negative log-likelihood, the valid count), optionally the argmax map and the confusion counts; (b) ONE workgroup adds the rows in double
//                       and writes the `stats` vector (losses, 1 / D and the gradient table u_k, v_k);
//   lmv_dense_loss_bwd: ONE pass that re-reads logits and labels and writes every element of dlogits once from that table.
// A pixel's classes are K planes a whole image apart: a thread owns a CHUNK of 16 bytes of consecutive pixels (4 fp32 / 8 bf16) and reads one 16-byte word per class
// plane where base and strides allow, element loads otherwise.  The chunks, the arithmetic behind the loads and every summation order are the same on both paths.
// No floating-point atomics: per-thread partials, a butterfly per wave, waves in order, rows in order.  Counts that go through atomics are integers.
#include <math.h>
#include <algorithm>
#include "common.h"

// one expression must give one value wherever the compiler places it (the vector and the element path share the code behind the loads)
#pragma clang fp contract(off)

namespace {
constexpr int DN_MAX_WG = 1024;          // workgroups of the forward pass: more chunks than DN_MAX_WG * threads are taken in further sweeps of the grid-stride loop
constexpr int DN_MAX_WG_BWD = 2048;
constexpr int DN_KREG = 5;               // K <= DN_KREG: class values and partial sums in registers; above: values re-read from cache, partial sums in LDS

struct DenseArgs {
  const void* logits; const void* labels; const float* alpha;
  float* ws; uint8_t* pred; unsigned long long* conf;
  const float* stats; const float* gout; void* dlogits;
  int64_t sb, sc, ignore, nchunks;
  int B, K, HW, cpi;          // cpi: chunks per image
  int xvec, lvec, pvec, dvec;          // 16-byte logits loads / vector label loads / vector pred stores / 16-byte dlogits stores are possible for FULL chunks
  float gamma, w_ce;
  int shape_terms;          // w_dice or w_jac is not 0: the u / v table matters
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

// ---- (a) the forward pass ---------------------------------------------------------------------------------------------------------------------------
// LDS (dynamic): KT > 0: red [waves][3 KT + 3] floats | conf [K K] ints;  KT == 0: accP [K][threads] | accI [K][threads] floats | cntT [K] ints | red [waves][3] | conf
template <typename T, typename LT, int KT> __global__ __launch_bounds__(256) void dense_fwd_kernel(const DenseArgs a) {
  constexpr int V = DT<T>::EPC;
  constexpr int KR = KT > 0 ? KT : 1;
  extern __shared__ float smem[];
  const int K = KT > 0 ? KT : a.K;
  const int NT = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  float* accP = smem;
  float* accI = smem + (KT > 0 ? 0 : K * NT);
  int* cntT = reinterpret_cast<int*>(smem + (KT > 0 ? 0 : 2 * K * NT));
  float* red = smem + (KT > 0 ? 0 : 2 * K * NT + K);
  int* conf = reinterpret_cast<int*>(red + (KT > 0 ? nw * (3 * KT + 3) : nw * 3));
  if (KT == 0) {
    for (int i = tid; i < 2 * K * NT; i += NT) smem[i] = 0.f;
    for (int i = tid; i < K; i += NT) cntT[i] = 0;
  }
  if (a.conf)
    for (int i = tid; i < K * K; i += NT) conf[i] = 0;
  __syncthreads();

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
    float mx[V], se[V], zy[V], py[V];
    int bi[V];
    if constexpr (KT > 0) {
      float z[KT][V];
#pragma unroll
      for (int k = 0; k < KT; ++k) dn_load<T>(x + k * a.sc, a.xvec && full, c.n, z[k]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float best = z[0][j], m = z[0][j];
        int b = 0;
#pragma unroll
        for (int k = 1; k < KT; ++k) {
          if (dn_better(z[k][j], best)) { best = z[k][j]; b = k; }
          m = fmaxf(m, z[k][j]);
        }
        bi[j] = b; mx[j] = m;
        float s = 0.f;
        zy[j] = 0.f; py[j] = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {          // z now holds the exponentials
          const float dz = z[k][j] - m;
          if (y[j] == k) zy[j] = dz;          // z_y - max
          z[k][j] = expf(dz); s += z[k][j];
        }
        se[j] = s;
        const float inv = 1.f / s;
        const bool on = y[j] >= 0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const float p = z[k][j] * inv;
          const bool hit = y[j] == k;
          if (on) rP[k] += p;
          if (hit) { rI[k] += p; rT[k] += 1; py[j] = p; }
        }
      }
    } else {
      float f[V];
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
          if (y[j] == k) { accI[k * NT + tid] += p; atomicAdd(&cntT[k], 1); zy[j] = f[j] - mx[j]; py[j] = p; }
        }
        accP[k * NT + tid] = sp;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (y[j] >= 0) {
        const float nll = logf(se[j]) - zy[j];          // -log p_y = log(sum exp(z - max)) - (z_y - max)
        ce_sum += dn_focal(a.alpha, a.gamma, y[j], py[j]) * nll;
        nll_sum += nll;
        nvalid += 1;
        if (a.conf) atomicAdd(&conf[y[j] * K + bi[j]], 1);
      }
    }
    if (a.pred) {
      uint8_t* pp = a.pred + c.poff;
      if (a.pvec && full) {
        if (V == 4) {
          *reinterpret_cast<uint32_t*>(pp) = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
        } else {
          uint32_t w[2] = {0u, 0u};
#pragma unroll
          for (int j = 0; j < V; ++j) w[j >> 2] |= (uint32_t)bi[j] << (8 * (j & 3));
          *reinterpret_cast<uint2*>(pp) = make_uint2(w[0], w[1]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (j < c.n) pp[j] = (uint8_t)bi[j];
      }
    }
  }

  // ---- the workgroup's row: butterfly per wave, waves in order ----
  float* row = a.ws + (int64_t)blockIdx.x * (3 * K + 3);
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
  if (a.conf) {          // (after a __syncthreads on either path) integer adds commute: the matrix does not depend on their order
    for (int i = tid; i < K * K; i += NT) {
      const int cnt = conf[i];
      if (cnt) atomicAdd(&a.conf[i], (unsigned long long)cnt);
    }
  }
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
        float py = 0.f, sg = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          z[k][j] = z[k][j] * inv;          // p_k
          const bool hit = y[j] == k;
          if (hit) py = z[k][j];
          if (a.shape_terms) sg += z[k][j] * (Vt[k] + (hit ? U[k] : 0.f));
        }
        const bool on = y[j] >= 0;
        const float cf = on ? a.w_ce * dn_focal(a.alpha, a.gamma, y[j], py) * invD : 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const bool hit = y[j] == k;
          float g = cf * (z[k][j] - (hit ? 1.f : 0.f));
          if (a.shape_terms) g = z[k][j] * ((Vt[k] + (hit ? U[k] : 0.f)) - sg) + g;
          z[k][j] = on ? gout * g : 0.f;
        }
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
          if (a.shape_terms) sg[j] += p * (vk + (hit ? uk : 0.f));
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) cf[j] = y[j] >= 0 ? a.w_ce * dn_focal(a.alpha, a.gamma, y[j], py[j]) * invD : 0.f;
      for (int k = 0; k < K; ++k) {
        dn_load<T>(x + k * a.sc, a.xvec && full, c.n, f);
        const float uk = U[k], vk = Vt[k];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float p = expf(f[j] - mx[j]) * (1.f / se[j]);
          const bool hit = y[j] == k;
          float g = cf[j] * (p - (hit ? 1.f : 0.f));
          if (a.shape_terms) g = p * ((vk + (hit ? uk : 0.f)) - sg[j]) + g;
          f[j] = y[j] >= 0 ? gout * g : 0.f;
        }
        dn_store<T>(d + k * plane, a.dvec && full, c.n, f);
      }
    }
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

static DenseArgs dn_args(const void* logits, int dtype, int64_t sb, int64_t sc, int B, int K, int64_t HW, const void* labels, int label_dtype, int64_t ignore,
                         const float* alpha, float gamma, float w_ce, float w_dice, float w_jac) {
  const int V = dtype == LMV_F32 ? 4 : 8;
  DenseArgs a = {};
  a.logits = logits; a.labels = labels; a.alpha = alpha;
  a.sb = sb; a.sc = sc; a.ignore = ignore;
  a.B = B; a.K = K; a.HW = (int)HW; a.cpi = (int)dn_cdiv(HW, V);
  a.nchunks = (int64_t)B * a.cpi;
  a.xvec = lmv_aligned16(logits) && sb % V == 0 && sc % V == 0;
  a.lvec = lmv_aligned16(labels) && HW % V == 0;
  a.gamma = gamma; a.w_ce = w_ce; a.shape_terms = (w_dice != 0.f || w_jac != 0.f) ? 1 : 0;
  return a;
}

#define DN_FOR_K(KERNEL, T, LT, ...)                                                              \
  switch (a.K <= DN_KREG ? a.K : 0) {                                                             \
    case 2: hipLaunchKernelGGL((KERNEL<T, LT, 2>), __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL((KERNEL<T, LT, 3>), __VA_ARGS__); break;                           \
    case 4: hipLaunchKernelGGL((KERNEL<T, LT, 4>), __VA_ARGS__); break;                           \
    case 5: hipLaunchKernelGGL((KERNEL<T, LT, 5>), __VA_ARGS__); break;                           \
    default: hipLaunchKernelGGL((KERNEL<T, LT, 0>), __VA_ARGS__); break;                          \
  }
#define DN_DISPATCH(KERNEL, ...)                                                                  \
  do {                                                                                            \
    if (dtype == LMV_F32) {                                                                       \
      if (label_dtype == LMV_DENSE_LABEL_I64) { DN_FOR_K(KERNEL, float, int64_t, __VA_ARGS__) }   \
      else { DN_FOR_K(KERNEL, float, uint8_t, __VA_ARGS__) }                                      \
    } else {                                                                                      \
      if (label_dtype == LMV_DENSE_LABEL_I64) { DN_FOR_K(KERNEL, bf16_t, int64_t, __VA_ARGS__) }  \
      else { DN_FOR_K(KERNEL, bf16_t, uint8_t, __VA_ARGS__) }                                     \
    }                                                                                             \
  } while (0)
}  // namespace

extern "C" size_t lmv_dense_loss_workspace_bytes(int B, int K, int64_t HW) {
  if (B < 1 || HW < 1 || K < 2 || K > LMV_DENSE_MAX_CLASSES || (int64_t)B * HW >= (1ll << 31)) return 0;
  return (size_t)dn_rows(B, K, HW, 4, DN_MAX_WG) * (size_t)(3 * K + 3) * sizeof(float);          // (bf16: 8 pixels per chunk, fewer rows)
}

extern "C" int lmv_dense_loss_fwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels,
                                  int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps,
                                  int avg_mode, void* workspace, size_t workspace_bytes, float* stats, uint8_t* pred, int64_t* conf, double* meter, void* stream) {
  if (int rc = dn_validate("dense_loss_fwd", logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, alpha, gamma, w_ce, w_dice, w_jac, eps, avg_mode)) return rc;
  if (!workspace || !stats) LMV_FAIL(LMV_ERR_SHAPE, "dense_loss_fwd: null workspace / stats");
  if ((((uintptr_t)workspace) & 3u) || (((uintptr_t)stats) & 3u) || (((uintptr_t)conf) & 7u) || (((uintptr_t)meter) & 7u)) LMV_FAIL(LMV_ERR_SHAPE, "dense_loss_fwd: misaligned buffer");
  const int V = dtype == LMV_F32 ? 4 : 8;
  const int rows = dn_rows(B, K, HW, V, DN_MAX_WG), NT = dn_threads(K);
  if (workspace_bytes < (size_t)rows * (size_t)(3 * K + 3) * sizeof(float))
    LMV_FAIL(LMV_ERR_SHAPE, "dense_loss_fwd: workspace of %zu bytes, %zu needed (lmv_dense_loss_workspace_bytes)", workspace_bytes, (size_t)rows * (size_t)(3 * K + 3) * sizeof(float));
  DenseArgs a = dn_args(logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.ws = reinterpret_cast<float*>(workspace); a.pred = pred; a.conf = reinterpret_cast<unsigned long long*>(conf);
  a.pvec = pred && (((uintptr_t)pred) & 7u) == 0 && HW % V == 0;
  const int nw = NT / 64;
  const size_t lds = (K <= DN_KREG ? (size_t)nw * (3 * K + 3) : (size_t)2 * K * NT + K + (size_t)nw * 3) * sizeof(float) + (conf ? (size_t)K * K * sizeof(int) : 0);
  hipStream_t st = (hipStream_t)stream;
  DN_DISPATCH(dense_fwd_kernel, dim3(rows), dim3(NT), lds, st, a);
  LMV_CHECK_LAUNCH("dense_loss_fwd");
  DenseFinArgs f;
  f.ws = a.ws; f.alpha = alpha; f.stats = stats; f.meter = meter; f.rows = rows; f.K = K; f.avg_mode = avg_mode;
  f.npix = (double)B * (double)HW; f.w_ce = w_ce; f.w_dice = w_dice; f.w_jac = w_jac; f.eps = eps;
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(1), dim3(256), 0, st, f);
  LMV_CHECK_LAUNCH("dense_loss_fwd (finalize)");
  return LMV_OK;
}

extern "C" int lmv_dense_loss_bwd(const void* logits, int dtype, int64_t batch_stride, int64_t class_stride, int B, int K, int64_t HW, const void* labels,
                                  int label_dtype, int64_t ignore_index, const float* alpha, float gamma, float w_ce, float w_dice, float w_jac, float eps,
                                  int avg_mode, const float* stats, const float* gout, void* dlogits, void* stream) {
  if (int rc = dn_validate("dense_loss_bwd", logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, alpha, gamma, w_ce, w_dice, w_jac, eps, avg_mode)) return rc;
  if (!stats || !dlogits) LMV_FAIL(LMV_ERR_SHAPE, "dense_loss_bwd: null stats / dlogits");
  if ((((uintptr_t)stats) & 3u) || (((uintptr_t)gout) & 3u) || (((uintptr_t)dlogits) & (dtype == LMV_F32 ? 3u : 1u))) LMV_FAIL(LMV_ERR_SHAPE, "dense_loss_bwd: misaligned buffer");
  const int V = dtype == LMV_F32 ? 4 : 8;
  DenseArgs a = dn_args(logits, dtype, batch_stride, class_stride, B, K, HW, labels, label_dtype, ignore_index, alpha, gamma, w_ce, w_dice, w_jac);
  a.stats = stats; a.gout = gout; a.dlogits = dlogits;
  a.dvec = lmv_aligned16(dlogits) && HW % V == 0;
  const int NT = 256, rows = (int)std::min<int64_t>(dn_cdiv(a.nchunks, NT), DN_MAX_WG_BWD);
  DN_DISPATCH(dense_bwd_kernel, dim3(rows), dim3(NT), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH("dense_loss_bwd");
  return LMV_OK;
}
